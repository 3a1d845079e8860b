// rtx_query.h — the launcher of the ray-query kernels (rtx_query.hip), shared with rtx_api.cpp.
//
// rtx_trace_rays / rtx_occluded_rays (include/rtx.h) trace rays the CALLER supplies: BoundingVolumeHierarchy::intersect
// (bounding_volume_hierarchy.rs:228) and the occlusion decision of main.rs:201-231 for a batch.  Their kernels live in a
// namespace of their own, rtxq: the statement "librtx.so's rtx:: kernels are the render pipeline's six" stays true.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "rtx_device.h"

namespace rtxq {

constexpr uint32_t kMaxRays = 1u << 28;      // ray numbers, 3 * n float offsets and 64-ray group numbers stay 32-bit
// Batches of fewer rays than this are traced in the caller's order unless the caller forces the regrouping pass
// (RTX_RAYS_FORCE_REGROUP): the key kernel and the radix sort are a fixed cost that a small batch cannot earn back.
// The figure is an estimate, not a measurement: tools/trace_rays_timing.py is the measurement it should come from
// (DESIGN.md "Ray queries").
constexpr uint32_t kRegroupMinRays = 1u << 14;

// The box the key kernel quantises origins in: lo and cells-per-unit of each axis (0 for a flat or non-finite axis).
struct KeyBox {
    float lo[3];
    float scale[3];
};
constexpr uint32_t kMortonBitsPerAxis = 9u;  // 27 bits of Morton code under the class bit and the three octant bits

// Buffers of the regrouping pass, n entries each, and rocprim's temporary storage; owned by the caller (DeviceState).
struct SortBuffers {
    uint32_t *keys, *keys_sorted, *index, *index_sorted;
    void     *temp;
    size_t    temp_bytes;
};
// temporary storage rocprim::radix_sort_pairs wants for n (key, index) pairs
hipError_t sort_temp_bytes(uint32_t n_entries, size_t *bytes);
// The regrouping pass, the one place librtx.so sorts: entry i of n_entries is keyed from ray i * stride of first / second
// (stride 1 for a list of rays, nb_ray for a list of pixels: a pixel is keyed by its ray 0; second_is_target: the
// direction is second - first), the (key, entry) pairs are sorted in `sort` (sized for n_entries at least), and *order
// is the list of entry numbers by rising key.
hipError_t regroup(uint32_t n_entries, uint32_t stride, const float *first, const float *second, bool second_is_target,
                   const KeyBox &box, const SortBuffers &sort, const uint32_t **order, hipStream_t stream);

// One batch.  first: n x 3 origins; second: n x 3 directions (closest hit) or targets (occlusion); out: n RtxRayHit
// (16-byte aligned) or n bytes; sort: NULL = trace in the caller's order; counters: NULL or rtx::kNumCounters words the
// kernels ADD to ([0] hits / occluded rays, [1..4] as the render kernels, [5] 64-ray groups that took the reference walk).
// origin_bound: the largest coordinate magnitude the multiply-based culling is proven for (PreparedScene::cull_delta *
// 2^19); a wavefront holding an origin beyond it walks with the exact slab test (rtx_ray_walk.hpp: origins_in_range).
hipError_t launch_query(const rtx::DeviceScene &S, bool occlusion, uint32_t n_rays, const float *first, const float *second,
                        const KeyBox &box, float origin_bound, const SortBuffers *sort, void *out,
                        unsigned long long *counters, hipStream_t stream);

}  // namespace rtxq
