// rtx_shade.hip — render_pixel for rays the CALLER supplies, for gfx950.
//
//   rtx_shade_rays      render_pixel's body (main.rs:186-236) per pixel, where create_rays returns the caller's nb_ray rays:
//                       closest hit (bvh.intersect), nb_light_sample shadow rays towards the scene's light points with the
//                       decision of main.rs:218-232, the sequential f32 sum, Color::to_rgba through the gamma thresholds
//
// A pixel is nb_ray consecutive rays of the caller's arrays.  One pixel per lane, 64 consecutive entries of the pixel list
// per wavefront — the caller's order, or the order of the regrouping pass (rtxq::regroup, rtx_query.hip: a pixel is keyed
// by its ray 0).  A result is written to the pixel's ORIGINAL number, so the order changes how long a batch takes and
// nothing else.
//
// The per-ray body — the walks, both votes, the shadow loop, the ordered sum — is rtx_shade_pixel.hpp's shade_ray, shared
// with rtx_view.hip.
//
// The kernels live in namespace rtxs: librtx.so's rtx:: kernels stay the render pipeline's six, its rtxq:: kernels the
// ray queries' nine.
#include "rtx_shade.h"
#include "rtx_shade_pixel.hpp"

namespace rtxs {

using namespace rtx;

// render_pixel (main.rs:180-240): one pixel per lane; lanes beyond n_pixels never vote.
// out_shade: one 16-byte word per pixel {avg_col.rgb as f32, bytes r, g, b, hits}; out_hits (may be NULL): closest_kernel's
// two 16-byte words per ray.
template <bool COUNT, bool SPHERES>
__global__ void __launch_bounds__(64 * kWavesPerGroup) shade_kernel(DeviceScene S, uint32_t n_pixels,
                                                                    const float *__restrict__ origins,
                                                                    const float *__restrict__ directions,
                                                                    const uint32_t *__restrict__ order,
                                                                    uint4 *__restrict__ out_shade,
                                                                    uint4 *__restrict__ out_hits,
                                                                    unsigned long long *__restrict__ counters,
                                                                    float origin_bound)
{
    uint32_t lane, pixel;
    bool active;
    if (!wave_entries(n_pixels, lane, pixel, active)) return;
    if (active && order) pixel = order[pixel];
    WalkTally tally;
    PixelSum sum;
    const float denom = (float)(S.nb_ray * S.nb_light);                              // main.rs:211
    for (uint32_t k = 0; k < S.nb_ray; ++k) {
        // the pixel's ray k, Ray::new(origin, direction) (ray.rs:15); lanes without a pixel carry a harmless regular one
        const size_t ray = (size_t)pixel * S.nb_ray + k;
        float ox = 0.0f, oy = 0.0f, oz = 0.0f, vx = 1.0f, vy = 1.0f, vz = 1.0f;
        if (active) {
            const float *a = origins + 3u * ray, *b = directions + 3u * ray;
            ox = a[0]; oy = a[1]; oz = a[2];
            vx = b[0]; vy = b[1]; vz = b[2];
        }
        shade_ray<COUNT, SPHERES>(S, active, k, ox, oy, oz, vx, vy, vz, origins_in_range(active, ox, oy, oz, origin_bound),
                                  origin_bound, denom, out_hits, ray, sum, tally);
    }
    if (active) out_shade[pixel] = pixel_word(sum, pixel_bytes(S, sum));
    if (COUNT) flush_tally(counters, lane, tally);
}

hipError_t launch_shade(const DeviceScene &S, uint32_t n_pixels, const float *origins, const float *directions,
                        const rtxq::KeyBox &box, float origin_bound, const rtxq::SortBuffers *sort, void *out_shade,
                        void *out_hits, unsigned long long *counters, hipStream_t stream)
{
    if (n_pixels == 0u) return hipSuccess;
    if (S.nb_ray == 0u || n_pixels > rtxq::kMaxRays / S.nb_ray) return hipErrorInvalidValue;
    const uint32_t *order = nullptr;
    if (sort) {
        const hipError_t e = rtxq::regroup(n_pixels, S.nb_ray, origins, directions, false, box, *sort, &order, stream);
        if (e != hipSuccess) return e;
    }
    launch_form(counters != nullptr, S.n_spheres != 0u, (n_pixels + 63u) / 64u, [&](auto count, auto spheres, dim3 grid, dim3 block) {
        hipLaunchKernelGGL((shade_kernel<count.value, spheres.value>), grid, block, 0, stream, S, n_pixels, origins, directions,
                           order, static_cast<uint4 *>(out_shade), static_cast<uint4 *>(out_hits), counters, origin_bound);
    });
    return hipGetLastError();
}

}  // namespace rtxs
