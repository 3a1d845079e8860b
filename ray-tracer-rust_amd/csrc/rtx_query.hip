// rtx_query.hip — ray queries for gfx950: closest hit and occlusion for rays the CALLER supplies.
//
//   rtx_trace_rays      BoundingVolumeHierarchy::intersect(&Ray::new(origin, direction)) per ray
//                       (bounding_volume_hierarchy.rs:50-75,228; ray.rs:12-17)
//   rtx_occluded_rays   the decision of main.rs:201-231 per (origin, target) pair
//
// The walk is rtx_traverse.hpp's, the one the render kernels use: one ray per lane, a wavefront walks the stream as ONE
// traversal.  Each wavefront owns 64 consecutive entries of the ray list — the caller's order, or the order of the
// regrouping pass (key_kernel + a radix sort of (key, ray number)), which puts rays of one direction octant and
// neighbouring origins into the same wavefront.  A result is written to the ray's ORIGINAL number, so the order changes
// how long a batch takes and nothing else.
//
// A 64-ray group holding a "hard" direction (a component -0.0, NaN or infinite: closest_hit / any_hit return false) is
// traced whole by closest_hit_reference — over the reference's own tree when the scene has it, else over the library's
// tree with ties by rank, which is reference_tiles_kernel's choice.
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
#include "rtx_traverse.hpp"

namespace rtxq {

using namespace rtx;

namespace {

constexpr uint32_t kWavesPerGroup = 4u;      // independent wavefronts: no barrier, no LDS
constexpr uint32_t kNoHit = 0xFFFFFFFFu;     // RTX_NO_HIT

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

// which stream a group with a hard ray walks (reference_tiles_kernel's choice)
__device__ __forceinline__ const NodeRec RTX_CONSTANT *reference_stream(const DeviceScene &S, uint32_t &n_stream, bool &have_ref)
{
    have_ref = S.n_ref_nodes != 0u;
    n_stream = have_ref ? S.n_ref_nodes : S.n_nodes;
    return (const NodeRec RTX_CONSTANT *)(have_ref ? S.ref_nodes : S.nodes);
}

__device__ __forceinline__ void add_counters(unsigned long long *__restrict__ counters, unsigned long long found,
                                             unsigned long long reference_groups, const WaveCounters &wc)
{
    if (!counters) return;
    if (found) atomicAdd(&counters[0], found);
    atomicAdd(&counters[1], wc.box_tests);
    atomicAdd(&counters[2], wc.tri_tests);
    atomicAdd(&counters[3], wc.node_visits);
    atomicAdd(&counters[4], wc.tri_visits);
    if (reference_groups) atomicAdd(&counters[5], reference_groups);
}

// The multiply-based culling of the walk (rtx_traverse.hpp: box_mask, advance_to_leaf) is a superset of the exact slab
// test because the stream's planes lie cull_delta = 2^-19 M further out, M the largest coordinate magnitude of the scene
// and the eye: that covers the plane distances' error, 3*2^-24 |P - o| + 1.01*2^-24 |o| + 2*2^-24 |p - o|, WHILE |o| <= M
// — true of every origin the render pipeline has (the eye, a hit point), not of a caller's (a pick ray from a distant
// camera).  origin_bound is that M; a wavefront holding a ray whose origin has a component beyond it (or a NaN: the
// comparison fails) walks with the exact slab test on the same, outward-moved, boxes — still a superset, no error term
// to cover, no pruning by distance.  One vote per wavefront.
__device__ __forceinline__ bool origins_in_range(bool active, float ox, float oy, float oz, float origin_bound)
{
    const bool inside = fabsf(ox) <= origin_bound && fabsf(oy) <= origin_bound && fabsf(oz) <= origin_bound;
    return ballot(active && !inside) == 0ull;
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

// One key per ray: bit 31 = the direction is hard (such rays share wavefronts: at most one group mixes the classes),
// bits 28-30 = the direction's octant (bit a: component a negative — advance_to_leaf has a loop per octant for wavefronts
// whose rays agree), bits 0-26 = Morton code of the origin's cell in the scene's box, clamped.  Also writes the identity
// the sort permutes.  The direction is Ray::new's (ray.rs:15), by square root and division: what the trace kernels get
// from length_and_direction, so the class here is the class there.
__global__ void __launch_bounds__(256) key_kernel(uint32_t n_rays, const float *__restrict__ first,
                                                  const float *__restrict__ second, uint32_t second_is_target, KeyBox box,
                                                  uint32_t *__restrict__ keys, uint32_t *__restrict__ index)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n_rays) return;
    const float *a = first + 3u * (size_t)i, *b = second + 3u * (size_t)i;
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

// Closest hit: one ray per lane, 64 consecutive entries of the list per wavefront; lanes beyond n_rays never vote.
// out: two 16-byte words per ray {prim, t, p_hit.x, p_hit.y} {p_hit.z, normal.xyz}; a miss is {RTX_NO_HIT, 0 ...}.
template <bool COUNT, bool SPHERES>
__global__ void __launch_bounds__(64 * kWavesPerGroup) closest_kernel(DeviceScene S, uint32_t n_rays,
                                                                      const float *__restrict__ origins,
                                                                      const float *__restrict__ directions,
                                                                      const uint32_t *__restrict__ order,
                                                                      uint4 *__restrict__ out,
                                                                      unsigned long long *__restrict__ counters,
                                                                      float origin_bound)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t group = __builtin_amdgcn_readfirstlane(blockIdx.x * kWavesPerGroup + (threadIdx.x >> 6));
    const uint32_t base = group << 6;            // n_rays <= 2^28 (rtxq::kMaxRays)
    if (base >= n_rays) return;                  // the whole wavefront
    const bool active = base + lane < n_rays;
    float ox, oy, oz, vx, vy, vz;
    const uint32_t ray = load_ray(base + lane, active, order, origins, directions, ox, oy, oz, vx, vy, vz);
    float len, dx, dy, dz;
    (void)length_and_direction(vx, vy, vz, len, dx, dy, dz);                        // Ray::new, ray.rs:15
    const TriRec RTX_CONSTANT *tris = (const TriRec RTX_CONSTANT *)S.tris;
    WaveCounters wc;
    LaneRay r = make_ray(active, ox, oy, oz, dx, dy, dz);
    unsigned long long reference_groups = 0;
    const NodeRec RTX_CONSTANT *nodes = (const NodeRec RTX_CONSTANT *)S.nodes;
    const bool walked = origins_in_range(active, ox, oy, oz, origin_bound)
                            ? closest_hit<COUNT, true, SPHERES>(nodes, tris, S.shade, S.n_nodes, r, wc, S.n_global)
                            : closest_hit<COUNT, false, SPHERES>(nodes, tris, S.shade, S.n_nodes, r, wc, S.n_global);
    if (!walked) {
        uint32_t n_stream;
        bool have_ref;
        const NodeRec RTX_CONSTANT *stream = reference_stream(S, n_stream, have_ref);
        closest_hit_reference<COUNT, SPHERES>(stream, tris, S.shade, n_stream, have_ref, active, ox, oy, oz, dx, dy, dz,
                                              r.best_t, r.best_idx, wc);
        reference_groups = 1;
    }
    const bool hit = active && r.best_idx != kNone;
    uint4 w0 = make_uint4(kNoHit, 0u, 0u, 0u), w1 = make_uint4(0u, 0u, 0u, 0u);
    if (hit) {
        const float t = r.best_t;
        const float hx = ox + t * dx, hy = oy + t * dy, hz = oz + t * dz;           // p_hit, bvh.rs:69
        const ShadeRec sh = S.shade[r.best_idx];
        float nx, ny, nz;
        hit_normal<SPHERES>(sh, hx, hy, hz, nx, ny, nz);                            // bvh.rs:72
        w0 = make_uint4(r.best_idx, __float_as_uint(t), __float_as_uint(hx), __float_as_uint(hy));
        w1 = make_uint4(__float_as_uint(hz), __float_as_uint(nx), __float_as_uint(ny), __float_as_uint(nz));
    }
    if (active) {
        out[2u * (size_t)ray] = w0;
        out[2u * (size_t)ray + 1u] = w1;
    }
    if (COUNT) {
        const unsigned long long found = __popcll(ballot(hit));
        if (lane == 0) add_counters(counters, found, reference_groups, wc);
    }
}

// Occlusion: the ray is Ray::new(origin, target - origin), D = distance(target, origin) (main.rs:201-202); it is occluded
// iff a closest hit exists and !(distance(origin, p_hit) > D) (main.rs:219-221) — which any_hit decides without finding
// the closest one (rtx_traverse.hpp: candidate_occludes).  out: one byte per ray, 1 = occluded.
template <bool COUNT, bool SPHERES>
__global__ void __launch_bounds__(64 * kWavesPerGroup) occluded_kernel(DeviceScene S, uint32_t n_rays,
                                                                       const float *__restrict__ origins,
                                                                       const float *__restrict__ targets,
                                                                       const uint32_t *__restrict__ order,
                                                                       uint8_t *__restrict__ out,
                                                                       unsigned long long *__restrict__ counters,
                                                                       float origin_bound)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t group = __builtin_amdgcn_readfirstlane(blockIdx.x * kWavesPerGroup + (threadIdx.x >> 6));
    const uint32_t base = group << 6;
    if (base >= n_rays) return;
    const bool active = base + lane < n_rays;
    float ox, oy, oz, tx, ty, tz;
    const uint32_t ray = load_ray(base + lane, active, order, origins, targets, ox, oy, oz, tx, ty, tz);
    const float vx = tx - ox, vy = ty - oy, vz = tz - oz;                           // p - orig, main.rs:201
    float dist, dx, dy, dz;
    (void)length_and_direction(vx, vy, vz, dist, dx, dy, dz);                       // main.rs:202, ray.rs:15
    const TriRec RTX_CONSTANT *tris = (const TriRec RTX_CONSTANT *)S.tris;
    WaveCounters wc;
    LaneRay r = make_ray(active, ox, oy, oz, dx, dy, dz);
    r.limit = dist;
    unsigned long long reference_groups = 0;
    bool occluded;
    const NodeRec RTX_CONSTANT *nodes = (const NodeRec RTX_CONSTANT *)S.nodes;
    const bool walked = origins_in_range(active, ox, oy, oz, origin_bound)
                            ? any_hit<COUNT, true, SPHERES>(nodes, tris, S.shade, S.n_nodes, r, wc, S.n_global)
                            : any_hit<COUNT, false, SPHERES>(nodes, tris, S.shade, S.n_nodes, r, wc, S.n_global);
    if (walked) {
        occluded = active && r.best_idx != kNone;
    } else {
        uint32_t n_stream, idx;
        bool have_ref;
        float t;
        const NodeRec RTX_CONSTANT *stream = reference_stream(S, n_stream, have_ref);
        closest_hit_reference<COUNT, SPHERES>(stream, tris, S.shade, n_stream, have_ref, active, ox, oy, oz, dx, dy, dz, t, idx, wc);
        occluded = false;
        if (active && idx != kNone) {
            const float qx = ox - (ox + t * dx), qy = oy - (oy + t * dy), qz = oz - (oz + t * dz);   // main.rs:220
            occluded = !(sqrtf(qx * qx + qy * qy + qz * qz) > dist);                                 // main.rs:221
        }
        reference_groups = 1;
    }
    if (active) out[ray] = occluded ? 1u : 0u;
    if (COUNT) {
        const unsigned long long found = __popcll(ballot(occluded));
        if (lane == 0) add_counters(counters, found, reference_groups, wc);
    }
}

hipError_t sort_temp_bytes(uint32_t n_rays, size_t *bytes)
{
    *bytes = 0;
    uint32_t *none = nullptr;
    return rocprim::radix_sort_pairs(nullptr, *bytes, none, none, none, none, n_rays, 0u, 32u, (hipStream_t) nullptr);
}

namespace {

template <bool COUNT, bool SPHERES>
void launch_form(const DeviceScene &S, bool occlusion, uint32_t n_rays, const float *first, const float *second,
                 const uint32_t *order, void *out, unsigned long long *counters, float origin_bound, hipStream_t stream)
{
    const uint32_t groups = (n_rays + 63u) / 64u;
    const dim3 grid((groups + kWavesPerGroup - 1u) / kWavesPerGroup), block(64u * kWavesPerGroup);
    if (occlusion)
        hipLaunchKernelGGL((occluded_kernel<COUNT, SPHERES>), grid, block, 0, stream, S, n_rays, first, second, order,
                           static_cast<uint8_t *>(out), counters, origin_bound);
    else
        hipLaunchKernelGGL((closest_kernel<COUNT, SPHERES>), grid, block, 0, stream, S, n_rays, first, second, order,
                           static_cast<uint4 *>(out), counters, origin_bound);
}

}  // namespace

hipError_t launch_query(const DeviceScene &S, bool occlusion, uint32_t n_rays, const float *first, const float *second,
                        const KeyBox &box, float origin_bound, const SortBuffers *sort, void *out,
                        unsigned long long *counters, hipStream_t stream)
{
    if (n_rays == 0u) return hipSuccess;
    if (n_rays > kMaxRays) return hipErrorInvalidValue;
    const uint32_t *order = nullptr;
    if (sort) {
        hipLaunchKernelGGL(key_kernel, dim3((n_rays + 255u) / 256u), dim3(256), 0, stream, n_rays, first, second,
                           occlusion ? 1u : 0u, box, sort->keys, sort->index);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
        size_t temp_bytes = sort->temp_bytes;
        e = rocprim::radix_sort_pairs(sort->temp, temp_bytes, sort->keys, sort->keys_sorted, sort->index, sort->index_sorted,
                                      n_rays, 0u, 32u, stream);
        if (e != hipSuccess) return e;
        order = sort->index_sorted;
    }
    const bool spheres = S.n_spheres != 0u;
    if (counters) {
        if (spheres) launch_form<true, true>(S, occlusion, n_rays, first, second, order, out, counters, origin_bound, stream);
        else launch_form<true, false>(S, occlusion, n_rays, first, second, order, out, counters, origin_bound, stream);
    } else {
        if (spheres) launch_form<false, true>(S, occlusion, n_rays, first, second, order, out, counters, origin_bound, stream);
        else launch_form<false, false>(S, occlusion, n_rays, first, second, order, out, counters, origin_bound, stream);
    }
    return hipGetLastError();
}

}  // namespace rtxq
