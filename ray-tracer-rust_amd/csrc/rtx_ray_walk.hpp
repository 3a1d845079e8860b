// rtx_ray_walk.hpp — what one wavefront of a ray-batch kernel does, stated once for rtxq::closest_kernel / occluded_kernel
// (rtx_query.hip), rtxs::shade_kernel (rtx_shade.hip) and rtxv::view_kernel (rtx_view.hip; the last two through
// rtx_shade_pixel.hpp's shade_ray): which 64 entries of the launch it owns, which of rtx_traverse.hpp's walks its 64 rays
// take — closest_hit / any_hit with the multiply-based or the exact box test, or closest_hit_reference when a direction is
// "hard" (a component -0.0, NaN or infinite: closest_hit / any_hit return false) — the hit record, and its counters.
// Also the launchers' choice of a kernel's COUNT x SPHERES form and grid.
#pragma once

#include <type_traits>

#include "rtx_device.h"
#include "rtx_traverse.hpp"

namespace rtx {

namespace {

constexpr uint32_t kWavesPerGroup = 4u;      // independent wavefronts: no barrier, no LDS
constexpr uint32_t kNoHit = 0xFFFFFFFFu;     // RTX_NO_HIT

// The wavefront's number in the launch (wave-uniform: a scalar) and the lane's number in the wavefront.
__device__ __forceinline__ uint32_t wave_of_launch(uint32_t &lane)
{
    lane = threadIdx.x & 63u;
    return __builtin_amdgcn_readfirstlane(blockIdx.x * kWavesPerGroup + (threadIdx.x >> 6));
}

// Wavefront g owns entries [64 g, 64 g + 64) of a list of n <= 2^28 (rtxq::kMaxRays).  false: none of them exists, the
// whole wavefront leaves.  slot: the lane's entry; active: it exists — lanes beyond n never vote.
__device__ __forceinline__ bool wave_entries(uint32_t n, uint32_t &lane, uint32_t &slot, bool &active)
{
    const uint32_t base = wave_of_launch(lane) << 6;
    slot = base + lane;
    active = slot < n;
    return base < n;
}

// what a wavefront counts (COUNT forms): the words of the launch's counter block it adds to
struct WalkTally {
    WaveCounters wc;                             // [1..4], as the render kernels
    unsigned long long found = 0;                // [0]: closest hits / occluded rays / primary hits
    unsigned long long reference_walks = 0;      // [5]: 64-lane walks that took the reference traversal
};

__device__ __forceinline__ void flush_tally(unsigned long long *__restrict__ counters, uint32_t lane, const WalkTally &t)
{
    if (lane != 0u || !counters) return;
    if (t.found) atomicAdd(&counters[0], t.found);
    atomicAdd(&counters[1], t.wc.box_tests);
    atomicAdd(&counters[2], t.wc.tri_tests);
    atomicAdd(&counters[3], t.wc.node_visits);
    atomicAdd(&counters[4], t.wc.tri_visits);
    if (t.reference_walks) atomicAdd(&counters[5], t.reference_walks);
}

// which stream a walk with a hard ray takes (reference_tiles_kernel's choice): the reference's own tree when the scene
// has it, else the library's tree with ties by rank
__device__ __forceinline__ const NodeRec RTX_CONSTANT *reference_stream(const DeviceScene &S, uint32_t &n_stream, bool &have_ref)
{
    have_ref = S.n_ref_nodes != 0u;
    n_stream = have_ref ? S.n_ref_nodes : S.n_nodes;
    return (const NodeRec RTX_CONSTANT *)(have_ref ? S.ref_nodes : S.nodes);
}

// The multiply-based culling of the walk (rtx_traverse.hpp: box_mask, advance_to_leaf) is a superset of the exact slab
// test because the stream's planes lie cull_delta = 2^-19 M further out, M the largest coordinate magnitude of the scene
// and the eye: that covers the plane distances' error, 3*2^-24 |P - o| + 1.01*2^-24 |o| + 2*2^-24 |p - o|, WHILE |o| <= M
// — true of every origin the render pipeline has (the eye, a hit point), not of a caller's (a pick ray from a distant
// camera).  origin_bound is that M; a wavefront holding a ray whose origin has a component beyond it (or a NaN: the
// comparison fails) walks with the exact slab test on the same, outward-moved, boxes — still a superset, no error term
// to cover, no pruning by distance.  One vote per 64-lane walk, handed to the helpers below as `in_range`: on the rays'
// origins for a primary walk (a kernel whose lanes share one origin knows the answer before it starts: rtx_view.hip), on
// the HIT POINTS for the shadow walks (a far origin's p_hit can round to just outside the bound although the scene lies
// inside it).
__device__ __forceinline__ bool origins_in_range(bool active, float ox, float oy, float oz, float origin_bound)
{
    const bool inside = fabsf(ox) <= origin_bound && fabsf(oy) <= origin_bound && fabsf(oz) <= origin_bound;
    return ballot(active && !inside) == 0ull;
}

// BoundingVolumeHierarchy::intersect(&Ray::new(o, v)) (bounding_volume_hierarchy.rs:50-75,228; ray.rs:15) for the
// wavefront's rays, one per lane; lanes that are not active carry a harmless regular ray and never vote.  d: Ray::new's
// direction; t, idx: the closest hit, idx == kNone for none.  Returns whether the lane has a hit; a reference walk is
// counted in the tally.
template <bool COUNT, bool SPHERES>
__device__ __forceinline__ bool closest_walk(const DeviceScene &S, bool active, bool in_range, float ox, float oy, float oz,
                                             float vx, float vy, float vz, float &dx, float &dy, float &dz, float &t,
                                             uint32_t &idx, WalkTally &tally)
{
    const TriRec RTX_CONSTANT *tris = (const TriRec RTX_CONSTANT *)S.tris;
    const NodeRec RTX_CONSTANT *nodes = (const NodeRec RTX_CONSTANT *)S.nodes;
    float len;
    (void)length_and_direction(vx, vy, vz, len, dx, dy, dz);                            // Ray::new, ray.rs:15
    LaneRay r = make_ray(active, ox, oy, oz, dx, dy, dz);
    const bool walked = in_range ? closest_hit<COUNT, true, SPHERES>(nodes, tris, S.shade, S.n_nodes, r, tally.wc, S.n_global)
                                 : closest_hit<COUNT, false, SPHERES>(nodes, tris, S.shade, S.n_nodes, r, tally.wc, S.n_global);
    if (!walked) {
        uint32_t n_stream;
        bool have_ref;
        const NodeRec RTX_CONSTANT *stream = reference_stream(S, n_stream, have_ref);
        closest_hit_reference<COUNT, SPHERES>(stream, tris, S.shade, n_stream, have_ref, active, ox, oy, oz, dx, dy, dz,
                                              r.best_t, r.best_idx, tally.wc);
        tally.reference_walks += 1;
    }
    t = r.best_t;
    idx = r.best_idx;
    return active && idx != kNone;
}

// The decision of main.rs:201-231 for the wavefront's (origin, target) pairs: the ray is Ray::new(o, v), v = target - o,
// D = |v| (main.rs:201-202); it is occluded iff a closest hit exists and !(distance(o, p_hit) > D) (main.rs:219-221) —
// which any_hit decides without finding the closest one (rtx_traverse.hpp: candidate_occludes).  d: Ray::new's direction.
// Returns the decision of a lane that is active — the caller masks the others, which a shadow loop does anyway — through
// one exit (with a second return in a branch the occlusion kernels came out longer); a reference walk is counted in the
// tally.
template <bool COUNT, bool SPHERES>
__device__ __forceinline__ bool occluded_walk(const DeviceScene &S, bool active, bool in_range, float ox, float oy, float oz,
                                              float vx, float vy, float vz, float &dx, float &dy, float &dz, WalkTally &tally)
{
    const TriRec RTX_CONSTANT *tris = (const TriRec RTX_CONSTANT *)S.tris;
    const NodeRec RTX_CONSTANT *nodes = (const NodeRec RTX_CONSTANT *)S.nodes;
    float dist;
    (void)length_and_direction(vx, vy, vz, dist, dx, dy, dz);                           // main.rs:202, ray.rs:15
    LaneRay r = make_ray(active, ox, oy, oz, dx, dy, dz);
    r.limit = dist;
    bool occluded;
    const bool walked = in_range ? any_hit<COUNT, true, SPHERES>(nodes, tris, S.shade, S.n_nodes, r, tally.wc, S.n_global)
                                 : any_hit<COUNT, false, SPHERES>(nodes, tris, S.shade, S.n_nodes, r, tally.wc, S.n_global);
    if (walked) {
        occluded = r.best_idx != kNone;
    } else {
        uint32_t n_stream, idx;
        bool have_ref;
        float t;
        const NodeRec RTX_CONSTANT *stream = reference_stream(S, n_stream, have_ref);
        closest_hit_reference<COUNT, SPHERES>(stream, tris, S.shade, n_stream, have_ref, active, ox, oy, oz, dx, dy, dz, t,
                                              idx, tally.wc);
        occluded = false;
        if (idx != kNone) {
            const float qx = ox - (ox + t * dx), qy = oy - (oy + t * dy), qz = oz - (oz + t * dz);   // main.rs:220
            occluded = !(sqrtf(qx * qx + qy * qy + qz * qz) > dist);                                 // main.rs:221
        }
        tally.reference_walks += 1;
    }
    return occluded;
}

// What intersect returns for a lane's closest hit (bvh.rs:66-74): p_hit, the normal and the primitive's colour — zeros
// for a miss — and the ray's record, two 16-byte words {prim, t, p_hit.x, p_hit.y} {p_hit.z, normal.xyz}; a miss is
// {RTX_NO_HIT, 0 ...}.
struct HitPoint {
    float x = 0.0f, y = 0.0f, z = 0.0f, nx = 0.0f, ny = 0.0f, nz = 0.0f, r = 0.0f, g = 0.0f, b = 0.0f;
    uint4 w0 = make_uint4(kNoHit, 0u, 0u, 0u), w1 = make_uint4(0u, 0u, 0u, 0u);
};

template <bool SPHERES>
__device__ __forceinline__ HitPoint hit_point(const DeviceScene &S, bool hit, float ox, float oy, float oz, float dx, float dy,
                                              float dz, float t, uint32_t idx)
{
    HitPoint h;
    if (hit) {
        h.x = ox + t * dx; h.y = oy + t * dy; h.z = oz + t * dz;                        // p_hit, bvh.rs:69
        const ShadeRec sh = S.shade[idx];
        hit_normal<SPHERES>(sh, h.x, h.y, h.z, h.nx, h.ny, h.nz);                       // bvh.rs:72
        h.r = sh.rgb[0]; h.g = sh.rgb[1]; h.b = sh.rgb[2];
        h.w0 = make_uint4(idx, __float_as_uint(t), __float_as_uint(h.x), __float_as_uint(h.y));
        h.w1 = make_uint4(__float_as_uint(h.z), __float_as_uint(h.nx), __float_as_uint(h.ny), __float_as_uint(h.nz));
    }
    return h;
}

__device__ __forceinline__ void store_hit(uint4 *__restrict__ out, size_t record, const HitPoint &h)
{
    out[2u * record] = h.w0;
    out[2u * record + 1u] = h.w1;
}

// Host side: launch the COUNT x SPHERES form of a kernel over n_waves wavefronts.  `launch(count, spheres, grid, block)`
// is called once, the two choices as std::bool_constant.
template <typename Launch>
void launch_form(bool count, bool spheres, uint32_t n_waves, Launch &&launch)
{
    const dim3 grid((n_waves + kWavesPerGroup - 1u) / kWavesPerGroup), block(64u * kWavesPerGroup);
    const auto with_count = [&](auto c) {
        if (spheres) launch(c, std::true_type{}, grid, block);
        else launch(c, std::false_type{}, grid, block);
    };
    if (count) with_count(std::true_type{});
    else with_count(std::false_type{});
}

}  // namespace

}  // namespace rtx
