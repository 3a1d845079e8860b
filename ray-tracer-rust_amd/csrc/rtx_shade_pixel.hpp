// rtx_shade_pixel.hpp — render_pixel's body (main.rs:186-236) for ONE ray per lane, whoever made the ray: the one statement
// of it that rtxs::shade_kernel (rtx_shade.hip: the caller's arrays) and rtxv::view_kernel (rtx_view.hip: a pinhole camera's
// rays, made in registers) both call, once per ray of their pixel.
//
// The walks, the votes that choose them, the hit record and the counters are rtx_ray_walk.hpp's, shared with the ray-query
// kernels (rtx_query.hip): closest_walk for the primary ray, occluded_walk with the light point as the target for a shadow
// ray.  The origin vote is taken twice: on the rays' origins for the primary walk (by the caller) and here on the HIT
// POINTS for the shadow walks (rtx_ray_walk.hpp: origins_in_range).
#pragma once

#include "rtx_ray_walk.hpp"

namespace rtx {

namespace {

// byte of a linear channel: number of thresholds (b >= 1) that are <= x  (color.rs:28-33); the render kernels' search,
// -inf counted as +inf as there (powf(-inf, 1 / 2.2) = +inf)
__device__ __forceinline__ uint32_t shade_quantise(const float *__restrict__ thr, float x)
{
    if (x == -__builtin_inff()) x = __builtin_inff();
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

// Ray k of the lane's pixel: Ray::new(origin, v) (ray.rs:15), the closest hit, the shadow rays towards light points
// [k][0..nb_light), the ordered sum into `px`.  active: the lane has a pixel (the others carry a harmless regular ray and
// never vote); origins_ok: wave-uniform, no active lane's origin lies beyond origin_bound; out_hits (may be NULL): the ray's
// hit record (closest_kernel's) goes to record `slot` of it.
template <bool COUNT, bool SPHERES>
__device__ __forceinline__ void shade_ray(const DeviceScene &S, bool active, uint32_t k, float ox, float oy, float oz, float vx,
                                          float vy, float vz, bool origins_ok, float origin_bound, float denom,
                                          uint4 *__restrict__ out_hits, size_t slot, PixelSum &px, WalkTally &tally)
{
    const float RTX_CONSTANT *lights = (const float RTX_CONSTANT *)S.light_points;   // wave-uniform reads: scalar operands
    float dx, dy, dz, t;
    uint32_t idx;
    const bool hit = closest_walk<COUNT, SPHERES>(S, active, origins_ok, ox, oy, oz, vx, vy, vz, dx, dy, dz, t, idx, tally);
    const HitPoint h = hit_point<SPHERES>(S, hit, ox, oy, oz, dx, dy, dz, t, idx);
    if (out_hits && active) store_hit(out_hits, slot, h);
    const unsigned long long hit_mask = ballot(hit);
    if (hit_mask == 0ull) return;                                                // main.rs:188: every lane's `None` arm
    if (COUNT) tally.found += __popcll(hit_mask);
    if (hit && px.n_hit < 255u) ++px.n_hit;
    const bool hits_in_range = origins_in_range(hit, h.x, h.y, h.z, origin_bound);
    for (uint32_t i = 0; i < S.nb_light; ++i) {                                  // main.rs:193
        const float RTX_CONSTANT *lp = lights + 3u * (k * S.nb_light + i);       // main.rs:194-196 (hoisted to the host)
        const bool occluded = occluded_walk<COUNT, SPHERES>(S, hit, hits_in_range, h.x, h.y, h.z, lp[0] - h.x, lp[1] - h.y,
                                                            lp[2] - h.z, dx, dy, dz, tally);   // p - p_hit, main.rs:201
        const float lnd = fabsf(h.nx * dx + h.ny * dy + h.nz * dz);              // main.rs:207
        // an occluded sample adds (black * 1.0) / denom = +0.0 (main.rs:226): left out, as shade_tiles_kernel leaves it out
        if (hit && !occluded) {
            px.r = px.r + ((h.r * lnd) / denom);                                 // main.rs:211-215
            px.g = px.g + ((h.g * lnd) / denom);
            px.b = px.b + ((h.b * lnd) / denom);
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

}  // namespace

}  // namespace rtx
