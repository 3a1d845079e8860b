// rtx_shade_pixel.hpp — render_pixel's body (main.rs:186-236) for ONE ray per lane, whoever made the ray: the one statement
// of it that rtxs::shade_kernel (rtx_shade.hip: the caller's arrays) and rtxv::view_kernel (rtx_view.hip: a pinhole camera's
// rays, made in registers) both call, once per ray of their pixel.
//
// The walks are rtx_traverse.hpp's, chosen as the ray-query kernels choose them (rtx_query.hip): closest_hit for the
// primary ray, any_hit with limit = distance to the light point for a shadow ray; a 64-lane walk holding a "hard"
// direction goes through closest_hit_reference; a walk holding an origin beyond origin_bound uses the exact slab test.
// That last vote is taken twice: on the rays' origins for the primary walk (by the caller: a kernel whose lanes share one
// origin knows the answer before it starts) and here on the HIT POINTS for the shadow walks (a far origin's p_hit can
// round to just outside the bound although the scene lies inside it).
#pragma once

#include "rtx_device.h"
#include "rtx_traverse.hpp"

namespace rtx {

namespace {

constexpr uint32_t kShadeNoHit = 0xFFFFFFFFu;    // RTX_NO_HIT

// which stream a walk with a hard ray takes (reference_tiles_kernel's choice)
__device__ __forceinline__ const NodeRec RTX_CONSTANT *reference_stream(const DeviceScene &S, uint32_t &n_stream, bool &have_ref)
{
    have_ref = S.n_ref_nodes != 0u;
    n_stream = have_ref ? S.n_ref_nodes : S.n_nodes;
    return (const NodeRec RTX_CONSTANT *)(have_ref ? S.ref_nodes : S.nodes);
}

// the multiply-based culling is proven for origins within origin_bound (rtx_query.hip: origins_in_range); one vote per walk
__device__ __forceinline__ bool origins_in_range(bool active, float ox, float oy, float oz, float origin_bound)
{
    const bool inside = fabsf(ox) <= origin_bound && fabsf(oy) <= origin_bound && fabsf(oz) <= origin_bound;
    return ballot(active && !inside) == 0ull;
}

// byte of a linear channel: number of thresholds (b >= 1) that are <= x  (color.rs:28-33); the render kernels' search
__device__ __forceinline__ uint32_t shade_quantise(const float *__restrict__ thr, float x)
{
    uint32_t b = 0;
#pragma unroll
    for (uint32_t step = 128; step; step >>= 1)
        if (x >= thr[b + step]) b += step;
    return b;
}

// what a lane keeps of its pixel between the pixel's rays
struct PixelSum {
    float r = 0.0f, g = 0.0f, b = 0.0f;          // avg_col, main.rs:182
    uint32_t n_hit = 0;                          // rays with a closest hit
};

// what a wavefront counts (COUNT forms)
struct ShadeTally {
    WaveCounters wc;
    unsigned long long primary_hits = 0, reference_walks = 0;
};

// Ray k of the lane's pixel: Ray::new(origin, v) (ray.rs:15), the closest hit, the shadow rays towards light points
// [k][0..nb_light), the ordered sum into `px`.  active: the lane has a pixel (the others carry a harmless regular ray and
// never vote); origins_ok: wave-uniform, no active lane's origin lies beyond origin_bound; out_hits (may be NULL): the ray's
// two 16-byte hit words (closest_kernel's record) go to record `slot` of it.
template <bool COUNT, bool SPHERES>
__device__ __forceinline__ void shade_ray(const DeviceScene &S, bool active, uint32_t k, float ox, float oy, float oz, float vx,
                                          float vy, float vz, bool origins_ok, float origin_bound, float denom,
                                          uint4 *__restrict__ out_hits, size_t slot, PixelSum &px, ShadeTally &tally)
{
    const TriRec RTX_CONSTANT *tris = (const TriRec RTX_CONSTANT *)S.tris;
    const NodeRec RTX_CONSTANT *nodes = (const NodeRec RTX_CONSTANT *)S.nodes;
    const float RTX_CONSTANT *lights = (const float RTX_CONSTANT *)S.light_points;   // wave-uniform reads: scalar operands
    WaveCounters &wc = tally.wc;
    float hx = 0.0f, hy = 0.0f, hz = 0.0f, nx = 0.0f, ny = 0.0f, nz = 0.0f, cr = 0.0f, cg = 0.0f, cb = 0.0f;
    bool hit;
    {
        float len, dx, dy, dz;
        (void)length_and_direction(vx, vy, vz, len, dx, dy, dz);
        LaneRay r = make_ray(active, ox, oy, oz, dx, dy, dz);
        const bool walked = origins_ok ? closest_hit<COUNT, true, SPHERES>(nodes, tris, S.shade, S.n_nodes, r, wc, S.n_global)
                                       : closest_hit<COUNT, false, SPHERES>(nodes, tris, S.shade, S.n_nodes, r, wc, S.n_global);
        if (!walked) {
            uint32_t n_stream;
            bool have_ref;
            const NodeRec RTX_CONSTANT *stream = reference_stream(S, n_stream, have_ref);
            closest_hit_reference<COUNT, SPHERES>(stream, tris, S.shade, n_stream, have_ref, active, ox, oy, oz, dx, dy, dz,
                                                  r.best_t, r.best_idx, wc);
            tally.reference_walks += 1;
        }
        hit = active && r.best_idx != kNone;
        uint4 w0 = make_uint4(kShadeNoHit, 0u, 0u, 0u), w1 = make_uint4(0u, 0u, 0u, 0u);
        if (hit) {
            const float t = r.best_t;
            hx = ox + t * dx; hy = oy + t * dy; hz = oz + t * dz;                // p_hit, bvh.rs:69
            const ShadeRec sh = S.shade[r.best_idx];
            hit_normal<SPHERES>(sh, hx, hy, hz, nx, ny, nz);                     // bvh.rs:72
            cr = sh.rgb[0]; cg = sh.rgb[1]; cb = sh.rgb[2];
            w0 = make_uint4(r.best_idx, __float_as_uint(t), __float_as_uint(hx), __float_as_uint(hy));
            w1 = make_uint4(__float_as_uint(hz), __float_as_uint(nx), __float_as_uint(ny), __float_as_uint(nz));
        }
        if (out_hits && active) {
            out_hits[2u * slot] = w0;
            out_hits[2u * slot + 1u] = w1;
        }
    }
    const unsigned long long hit_mask = ballot(hit);
    if (hit_mask == 0ull) return;                                                // main.rs:188: every lane's `None` arm
    if (COUNT) tally.primary_hits += __popcll(hit_mask);
    if (hit && px.n_hit < 255u) ++px.n_hit;
    const bool hits_in_range = origins_in_range(hit, hx, hy, hz, origin_bound);
    for (uint32_t i = 0; i < S.nb_light; ++i) {                                  // main.rs:193
        const float RTX_CONSTANT *lp = lights + 3u * (k * S.nb_light + i);       // main.rs:194-196 (hoisted to the host)
        const float sx = lp[0] - hx, sy = lp[1] - hy, sz = lp[2] - hz;           // p - p_hit, main.rs:201
        float dist, dx, dy, dz;
        (void)length_and_direction(sx, sy, sz, dist, dx, dy, dz);                // main.rs:202, ray.rs:15
        LaneRay r = make_ray(hit, hx, hy, hz, dx, dy, dz);
        r.limit = dist;
        bool occluded;
        const bool walked = hits_in_range
                                ? any_hit<COUNT, true, SPHERES>(nodes, tris, S.shade, S.n_nodes, r, wc, S.n_global)
                                : any_hit<COUNT, false, SPHERES>(nodes, tris, S.shade, S.n_nodes, r, wc, S.n_global);
        if (walked) {
            occluded = r.best_idx != kNone;
        } else {
            uint32_t n_stream, idx;
            bool have_ref;
            float t;
            const NodeRec RTX_CONSTANT *stream = reference_stream(S, n_stream, have_ref);
            closest_hit_reference<COUNT, SPHERES>(stream, tris, S.shade, n_stream, have_ref, hit, hx, hy, hz, dx, dy, dz, t, idx, wc);
            occluded = false;
            if (idx != kNone) {
                const float qx = hx - (hx + t * dx), qy = hy - (hy + t * dy), qz = hz - (hz + t * dz);   // main.rs:220
                occluded = !(sqrtf(qx * qx + qy * qy + qz * qz) > dist);                                 // main.rs:221
            }
            tally.reference_walks += 1;
        }
        const float lnd = fabsf(nx * dx + ny * dy + nz * dz);                    // main.rs:207
        // an occluded sample adds (black * 1.0) / denom = +0.0 (main.rs:226): left out, as shade_tiles_kernel leaves it out
        if (hit && !occluded) {
            px.r = px.r + ((cr * lnd) / denom);                                  // main.rs:211-215
            px.g = px.g + ((cg * lnd) / denom);
            px.b = px.b + ((cb * lnd) / denom);
        }
    }
}

// Color::to_rgba of the sum through the gamma thresholds: bytes r, g, b and the hit count, RtxPixelShade's last word
__device__ __forceinline__ uint32_t pixel_bytes(const DeviceScene &S, const PixelSum &px)
{
    return shade_quantise(S.gamma_thr, px.r) | (shade_quantise(S.gamma_thr, px.g) << 8) |
           (shade_quantise(S.gamma_thr, px.b) << 16) | (px.n_hit << 24);
}

// one RtxPixelShade record
__device__ __forceinline__ uint4 pixel_word(const PixelSum &px, uint32_t bytes)
{
    return make_uint4(__float_as_uint(px.r), __float_as_uint(px.g), __float_as_uint(px.b), bytes);
}

// a wavefront's counts into the launch's counter block: one lane calls it
__device__ __forceinline__ void flush_tally(unsigned long long *__restrict__ counters, const ShadeTally &t)
{
    if (t.primary_hits) atomicAdd(&counters[0], t.primary_hits);
    atomicAdd(&counters[1], t.wc.box_tests);
    atomicAdd(&counters[2], t.wc.tri_tests);
    atomicAdd(&counters[3], t.wc.node_visits);
    atomicAdd(&counters[4], t.wc.tri_visits);
    if (t.reference_walks) atomicAdd(&counters[5], t.reference_walks);
}

}  // namespace

}  // namespace rtx
