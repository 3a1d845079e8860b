// rtx_query.hip — ray queries for gfx950: closest hit and occlusion for rays the CALLER supplies, and the regrouping pass
// of every ray-batch call.
//
//   rtx_trace_rays      BoundingVolumeHierarchy::intersect(&Ray::new(origin, direction)) per ray
//                       (bounding_volume_hierarchy.rs:50-75,228; ray.rs:12-17)
//   rtx_occluded_rays   the decision of main.rs:201-231 per (origin, target) pair
//
// The walk is rtx_traverse.hpp's, the one the render kernels use: one ray per lane, a wavefront walks the stream as ONE
// traversal.  Each wavefront owns 64 consecutive entries of the ray list — the caller's order, or the order of the
// regrouping pass (regroup: key_kernel + a radix sort of (key, entry number)), which puts rays of one direction octant and
// neighbouring origins into the same wavefront.  A result is written to the ray's ORIGINAL number, so the order changes
// how long a batch takes and nothing else.  rtx_shade_rays (rtx_shade.hip) regroups its pixels through the same regroup:
// this is the one translation unit that instantiates rocprim.
//
// What a wavefront does with its 64 rays — which walk, the hard-ray rule, the origin vote, the hit record, the counters —
// is rtx_ray_walk.hpp's, shared with the shading kernels.
//
// The kernels live in namespace rtxq, outside rtx: librtx.so's rtx:: kernels are the render pipeline's six and stay so.
#include <cstdlib>
#include <type_traits>
// librtx.so behaves the same whatever the caller's environment holds: it imports no getenv (tests/test_host_prep.py,
// tests/test_trace_rays_host.py — which is also what notices if a later rocprim reaches the environment another way).
// rocprim's host side asks for one tuning override, `std::getenv("ROCPRIM_USE_ATOMIC_BLOCK_ID")` (ordered_block_id.hpp);
// inside this translation unit that expression reads `std::add_pointer_t<char>(nullptr)` — a null char *, "not set",
// rocprim's default — so nothing is added to namespace std and libc is not reached.
#define getenv(name) add_pointer_t<char>(nullptr)
#include <rocprim/device/device_radix_sort.hpp>
#undef getenv

#include "rtx_query.h"
#include "rtx_ray_walk.hpp"

namespace rtxq {

using namespace rtx;

namespace {

// ray `slot` of the (possibly permuted) list: its original number and its two vectors; lanes without a ray carry a
// harmless regular one (they never vote, but length_and_direction's short way wants every lane in range)
__device__ __forceinline__ uint32_t load_ray(uint32_t slot, bool active, const uint32_t *__restrict__ order,
                                             const float *__restrict__ first, const float *__restrict__ second,
                                             float &ax, float &ay, float &az, float &bx, float &by, float &bz)
{
    uint32_t ray = slot;
    ax = ay = az = 0.0f;
    bx = by = bz = 1.0f;
    if (active) {
        if (order) ray = order[slot];
        const float *a = first + 3u * (size_t)ray, *b = second + 3u * (size_t)ray;
        ax = a[0]; ay = a[1]; az = a[2];
        bx = b[0]; by = b[1]; bz = b[2];
    }
    return ray;
}

// spreads the low nine bits of x to every third bit
__device__ __forceinline__ uint32_t spread3(uint32_t x)
{
    x &= 0x1FFu;
    x = (x | (x << 16)) & 0x030000FFu;
    x = (x | (x << 8)) & 0x0300F00Fu;
    x = (x | (x << 4)) & 0x030C30C3u;
    x = (x | (x << 2)) & 0x09249249u;
    return x;
}

__device__ __forceinline__ uint32_t cell(float x, float lo, float scale)
{
    const float c = fminf(fmaxf((x - lo) * scale, 0.0f), (float)((1u << kMortonBitsPerAxis) - 1u));   // a NaN ends as 0
    return (uint32_t)c;
}

}  // namespace

// One key per entry, from ray i * stride of the arrays (stride 1: every ray is an entry; stride nb_ray: an entry is a
// pixel, keyed by its ray 0): bit 31 = the direction is hard (such entries share wavefronts: at most one group mixes the
// classes), bits 28-30 = the direction's octant (bit a: component a negative — advance_to_leaf has a loop per octant for
// wavefronts whose rays agree), bits 0-26 = Morton code of the origin's cell in the scene's box, clamped.  Also writes
// the identity the sort permutes.  The direction is Ray::new's (ray.rs:15), by square root and division: what the trace
// kernels get from length_and_direction, so the class here is the class there.
__global__ void __launch_bounds__(256) key_kernel(uint32_t n_entries, uint32_t stride, const float *__restrict__ first,
                                                  const float *__restrict__ second, uint32_t second_is_target, KeyBox box,
                                                  uint32_t *__restrict__ keys, uint32_t *__restrict__ index)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n_entries) return;
    const float *a = first + 3u * ((size_t)i * stride), *b = second + 3u * ((size_t)i * stride);
    const float ox = a[0], oy = a[1], oz = a[2];
    float vx = b[0], vy = b[1], vz = b[2];
    if (second_is_target) { vx = vx - ox; vy = vy - oy; vz = vz - oz; }
    const float len = sqrtf(vx * vx + vy * vy + vz * vz);
    const float dx = vx / len, dy = vy / len, dz = vz / len;
    const uint32_t hard = direction_is_hard(dx, dy, dz) ? 1u : 0u;
    const uint32_t octant = (dx < 0.0f ? 1u : 0u) | (dy < 0.0f ? 2u : 0u) | (dz < 0.0f ? 4u : 0u);
    const uint32_t morton = spread3(cell(ox, box.lo[0], box.scale[0])) | (spread3(cell(oy, box.lo[1], box.scale[1])) << 1) |
                            (spread3(cell(oz, box.lo[2], box.scale[2])) << 2);
    keys[i] = (hard << 31) | (octant << 28) | morton;
    index[i] = i;
}

// Closest hit: one ray per lane, 64 consecutive entries of the list per wavefront.
// out: rtx_ray_walk.hpp's record, two 16-byte words per ray.
template <bool COUNT, bool SPHERES>
__global__ void __launch_bounds__(64 * kWavesPerGroup) closest_kernel(DeviceScene S, uint32_t n_rays,
                                                                      const float *__restrict__ origins,
                                                                      const float *__restrict__ directions,
                                                                      const uint32_t *__restrict__ order,
                                                                      uint4 *__restrict__ out,
                                                                      unsigned long long *__restrict__ counters,
                                                                      float origin_bound)
{
    uint32_t lane, slot, idx;
    bool active;
    if (!wave_entries(n_rays, lane, slot, active)) return;
    float ox, oy, oz, vx, vy, vz, dx, dy, dz, t;
    const uint32_t ray = load_ray(slot, active, order, origins, directions, ox, oy, oz, vx, vy, vz);
    WalkTally tally;
    const bool hit = closest_walk<COUNT, SPHERES>(S, active, origins_in_range(active, ox, oy, oz, origin_bound), ox, oy, oz,
                                                  vx, vy, vz, dx, dy, dz, t, idx, tally);
    const HitPoint h = hit_point<SPHERES>(S, hit, ox, oy, oz, dx, dy, dz, t, idx);
    if (active) store_hit(out, ray, h);
    if (COUNT) {
        tally.found = __popcll(ballot(hit));
        flush_tally(counters, lane, tally);
    }
}

// Occlusion: the decision of main.rs:201-231 per (origin, target) pair.  out: one byte per ray, 1 = occluded.
template <bool COUNT, bool SPHERES>
__global__ void __launch_bounds__(64 * kWavesPerGroup) occluded_kernel(DeviceScene S, uint32_t n_rays,
                                                                       const float *__restrict__ origins,
                                                                       const float *__restrict__ targets,
                                                                       const uint32_t *__restrict__ order,
                                                                       uint8_t *__restrict__ out,
                                                                       unsigned long long *__restrict__ counters,
                                                                       float origin_bound)
{
    uint32_t lane, slot;
    bool active;
    if (!wave_entries(n_rays, lane, slot, active)) return;
    float ox, oy, oz, tx, ty, tz, dx, dy, dz;
    const uint32_t ray = load_ray(slot, active, order, origins, targets, ox, oy, oz, tx, ty, tz);
    WalkTally tally;
    // (the walk is the whole wavefront's: called by every lane, and the lanes without a ray masked afterwards)
    const bool decision = occluded_walk<COUNT, SPHERES>(S, active, origins_in_range(active, ox, oy, oz, origin_bound), ox, oy, oz,
                                                        tx - ox, ty - oy, tz - oz, dx, dy, dz, tally);   // p - orig, main.rs:201
    const bool occluded = active && decision;
    if (active) out[ray] = occluded ? 1u : 0u;
    if (COUNT) {
        tally.found = __popcll(ballot(occluded));
        flush_tally(counters, lane, tally);
    }
}

hipError_t sort_temp_bytes(uint32_t n_entries, size_t *bytes)
{
    *bytes = 0;
    uint32_t *none = nullptr;
    return rocprim::radix_sort_pairs(nullptr, *bytes, none, none, none, none, n_entries, 0u, 32u, (hipStream_t) nullptr);
}

hipError_t regroup(uint32_t n_entries, uint32_t stride, const float *first, const float *second, bool second_is_target,
                   const KeyBox &box, const SortBuffers &sort, const uint32_t **order, hipStream_t stream)
{
    hipLaunchKernelGGL(key_kernel, dim3((n_entries + 255u) / 256u), dim3(256), 0, stream, n_entries, stride, first, second,
                       second_is_target ? 1u : 0u, box, sort.keys, sort.index);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    size_t temp_bytes = sort.temp_bytes;
    e = rocprim::radix_sort_pairs(sort.temp, temp_bytes, sort.keys, sort.keys_sorted, sort.index, sort.index_sorted, n_entries,
                                  0u, 32u, stream);
    *order = sort.index_sorted;
    return e;
}

hipError_t launch_query(const DeviceScene &S, bool occlusion, uint32_t n_rays, const float *first, const float *second,
                        const KeyBox &box, float origin_bound, const SortBuffers *sort, void *out,
                        unsigned long long *counters, hipStream_t stream)
{
    if (n_rays == 0u) return hipSuccess;
    if (n_rays > kMaxRays) return hipErrorInvalidValue;
    const uint32_t *order = nullptr;
    if (sort) {
        const hipError_t e = regroup(n_rays, 1u, first, second, occlusion, box, *sort, &order, stream);
        if (e != hipSuccess) return e;
    }
    launch_form(counters != nullptr, S.n_spheres != 0u, (n_rays + 63u) / 64u, [&](auto count, auto spheres, dim3 grid, dim3 block) {
        if (occlusion)
            hipLaunchKernelGGL((occluded_kernel<count.value, spheres.value>), grid, block, 0, stream, S, n_rays, first, second,
                               order, static_cast<uint8_t *>(out), counters, origin_bound);
        else
            hipLaunchKernelGGL((closest_kernel<count.value, spheres.value>), grid, block, 0, stream, S, n_rays, first, second,
                               order, static_cast<uint4 *>(out), counters, origin_bound);
    });
    return hipGetLastError();
}

}  // namespace rtxq
