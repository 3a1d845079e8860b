// rtx_view.hip — a rectangle of any pinhole view of an uploaded scene, for gfx950.
//
//   rtx_render_view     pixel (px, py) of the view gets render_pixel(px, py) (main.rs:180-240) of a reference Scene that has
//                       the view's width, height and camera and the uploaded scene's primitives, light, nb_ray,
//                       nb_light_sample and sample table
//
// One wavefront is one 8 x 8 tile of the RECTANGLE, tiles row by row over ceil(nx/8) x ceil(ny/8): lane l is pixel
// (x0 + 8*tx + (l & 7), y0 + 8*ty + (l >> 3)).  The rays of a tile leave one point towards neighbouring pixels, and its
// shadow rays towards one light point leave neighbouring hit points: the coherence the wave-uniform walk lives on, which
// rtx_shade_rays gets for caller-made rays only from its regrouping pass.  No sort runs here, and no ray array is read:
// a lane makes its rays in registers from the view block (kernel argument, wave-uniform; the eye is a scalar operand),
// with create_rays' arithmetic as rtx_pass_helpers.hpp's primary_ray has it.
//
// Four independent wavefronts per workgroup: no barrier, no LDS.  The per-ray body is rtx_shade_pixel.hpp's shade_ray,
// the one rtxs::shade_kernel calls: a view's records are byte for byte what rtx_shade_rays and rtx_trace_rays return for
// the same rays.  Every lane's origin is the eye, so the primary walks' origin vote is taken once, on the host.
//
// The kernels live in namespace rtxv: librtx.so's rtx::, rtxq:: and rtxs:: kernel sets stay what they were.
#include "rtx_view.h"
#include "rtx_shade_pixel.hpp"

namespace rtxv {

using namespace rtx;

// out_rgb (may be NULL): three bytes per pixel; out_shade (may be NULL): one 16-byte word per pixel {avg_col.rgb as f32,
// bytes r, g, b, hits}; out_hits (may be NULL): closest_kernel's two 16-byte words per ray.  Lanes outside the rectangle
// carry a harmless regular ray and never vote.
template <bool COUNT, bool SPHERES>
__global__ void __launch_bounds__(64 * kWavesPerGroup) view_kernel(DeviceScene S, ViewBlock V, uint32_t tiles_x, uint32_t n_tiles,
                                                                   uint8_t *__restrict__ out_rgb,
                                                                   uint4 *__restrict__ out_shade,
                                                                   uint4 *__restrict__ out_hits,
                                                                   unsigned long long *__restrict__ counters,
                                                                   float origin_bound, uint32_t eye_in_range)
{
    uint32_t lane;
    const uint32_t tile = wave_of_launch(lane);
    if (tile >= n_tiles) return;                 // the whole wavefront
    const uint32_t ty = tile / tiles_x, tx = tile - ty * tiles_x;
    const uint32_t lx = tx * 8u + (lane & 7u), ly = ty * 8u + (lane >> 3);
    const bool active = lx < V.nx && ly < V.ny;
    const uint32_t px = V.x0 + lx, py = V.y0 + ly;                                   // the pixel in the view's frame
    const size_t slot = (size_t)ly * V.nx + lx;                                      // ... and in the outputs: < 2^28
    WalkTally tally;
    PixelSum sum;
    const float denom = (float)(S.nb_ray * S.nb_light);                              // main.rs:211
    for (uint32_t k = 0; k < S.nb_ray; ++k) {
        // create_rays (main.rs:151-178) for ray k of pixel (px, py), up to Ray::new
        float s0 = 0.0f, s1 = 0.0f;
        if (active) {
            const float2 s = S.samples[(px * V.width + py + k) % S.n_samples];       // :162,165 (u32)
            s0 = s.x;
            s1 = s.y;
        }
        const float a = (float)px - (float)V.width / 2.0f + s0;                      // :161-162
        const float b = (float)py - (float)V.height / 2.0f + s1;                     // :164-165
        const float rx = (a * V.u[0] + b * V.v[0]) - V.distance * V.w[0];            // :160-167
        const float ry = (a * V.u[1] + b * V.v[1]) - V.distance * V.w[1];
        const float rz = (a * V.u[2] + b * V.v[2]) - V.distance * V.w[2];
        shade_ray<COUNT, SPHERES>(S, active, k, V.eye[0], V.eye[1], V.eye[2], active ? rx : 1.0f, active ? ry : 1.0f,
                                  active ? rz : 1.0f, eye_in_range != 0u, origin_bound, denom, out_hits, slot * S.nb_ray + k,
                                  sum, tally);
    }
    if (active) {
        const uint32_t bytes = pixel_bytes(S, sum);
        if (out_rgb) {
            uint8_t *p = out_rgb + slot * 3u;                                        // put_pixel, main.rs:293-294
            p[0] = (uint8_t)bytes;
            p[1] = (uint8_t)(bytes >> 8);
            p[2] = (uint8_t)(bytes >> 16);
        }
        if (out_shade) out_shade[slot] = pixel_word(sum, bytes);
    }
    if (COUNT) flush_tally(counters, lane, tally);
}

hipError_t launch_view(const DeviceScene &S, const ViewBlock &V, float origin_bound, void *d_rgb, void *d_shade, void *d_hits,
                       unsigned long long *counters, hipStream_t stream)
{
    if (V.nx == 0u || V.ny == 0u) return hipSuccess;
    const uint64_t rays = static_cast<uint64_t>(V.nx) * V.ny * S.nb_ray;
    if (S.nb_ray == 0u || S.n_samples == 0u || rays > kMaxRays) return hipErrorInvalidValue;
    const uint64_t tiles_x = (static_cast<uint64_t>(V.nx) + 7u) / 8u, tiles_y = (static_cast<uint64_t>(V.ny) + 7u) / 8u;
    const uint64_t n_tiles = tiles_x * tiles_y;      // <= (nx/8 + 1)(ny/8 + 1) <= 2^22 + 2^25 + 2
    if (n_tiles > 0x7FFFFFFFull) return hipErrorInvalidValue;
    // origins_in_range (rtx_ray_walk.hpp) for the one origin every lane has
    const bool eye_in_range = fabsf(V.eye[0]) <= origin_bound && fabsf(V.eye[1]) <= origin_bound && fabsf(V.eye[2]) <= origin_bound;
    launch_form(counters != nullptr, S.n_spheres != 0u, static_cast<uint32_t>(n_tiles), [&](auto count, auto spheres, dim3 grid, dim3 block) {
        hipLaunchKernelGGL((view_kernel<count.value, spheres.value>), grid, block, 0, stream, S, V, static_cast<uint32_t>(tiles_x),
                           static_cast<uint32_t>(n_tiles), static_cast<uint8_t *>(d_rgb), static_cast<uint4 *>(d_shade),
                           static_cast<uint4 *>(d_hits), counters, origin_bound, eye_in_range ? 1u : 0u);
    });
    return hipGetLastError();
}

}  // namespace rtxv
