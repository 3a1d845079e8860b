// rtx_shade.hip — render_pixel for rays the CALLER supplies, for gfx950.
//
//   rtx_shade_rays      render_pixel's body (main.rs:186-236) per pixel, where create_rays returns the caller's nb_ray rays:
//                       closest hit (bvh.intersect), nb_light_sample shadow rays towards the scene's light points with the
//                       decision of main.rs:218-232, the sequential f32 sum, Color::to_rgba through the gamma thresholds
//
// A pixel is nb_ray consecutive rays of the caller's arrays.  One pixel per lane, 64 consecutive entries of the pixel list
// per wavefront — the caller's order, or the order of the regrouping pass (key_kernel on each pixel's ray 0 + the radix
// sort rtx_query.hip uses, in the same buffers).  A result is written to the pixel's ORIGINAL number, so the order changes
// how long a batch takes and nothing else.
//
// The per-ray body — the walks, both votes, the shadow loop, the ordered sum — is rtx_shade_pixel.hpp's shade_ray, shared
// with rtx_view.hip.
//
// The kernels live in namespace rtxs: librtx.so's rtx:: kernels stay the render pipeline's six, its rtxq:: kernels the
// ray queries' nine.
#include <cstdlib>
#include <type_traits>
// (rtx_query.hip: librtx.so imports no getenv; rocprim's one `std::getenv(...)` reads as a null char * in here)
#define getenv(name) add_pointer_t<char>(nullptr)
#include <rocprim/device/device_radix_sort.hpp>
#undef getenv

#include "rtx_shade.h"
#include "rtx_shade_pixel.hpp"

namespace rtxs {

using namespace rtx;

namespace {

constexpr uint32_t kWavesPerGroup = 4u;      // independent wavefronts: no barrier, no LDS

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
    const float c = fminf(fmaxf((x - lo) * scale, 0.0f), (float)((1u << rtxq::kMortonBitsPerAxis) - 1u));   // a NaN ends as 0
    return (uint32_t)c;
}

}  // namespace

// One key per pixel, from its ray 0, laid out as rtxq::key_kernel's: bit 31 = the direction is hard, bits 28-30 = the
// direction's octant, bits 0-26 = Morton code of the origin's cell in the scene's box.  Also writes the identity the
// sort permutes.
__global__ void __launch_bounds__(256) key_kernel(uint32_t n_pixels, uint32_t nb_ray, const float *__restrict__ origins,
                                                  const float *__restrict__ directions, rtxq::KeyBox box,
                                                  uint32_t *__restrict__ keys, uint32_t *__restrict__ index)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n_pixels) return;
    const float *a = origins + 3u * ((size_t)i * nb_ray), *b = directions + 3u * ((size_t)i * nb_ray);
    const float ox = a[0], oy = a[1], oz = a[2];
    const float vx = b[0], vy = b[1], vz = b[2];
    const float len = sqrtf(vx * vx + vy * vy + vz * vz);
    const float dx = vx / len, dy = vy / len, dz = vz / len;
    const uint32_t hard = direction_is_hard(dx, dy, dz) ? 1u : 0u;
    const uint32_t octant = (dx < 0.0f ? 1u : 0u) | (dy < 0.0f ? 2u : 0u) | (dz < 0.0f ? 4u : 0u);
    const uint32_t morton = spread3(cell(ox, box.lo[0], box.scale[0])) | (spread3(cell(oy, box.lo[1], box.scale[1])) << 1) |
                            (spread3(cell(oz, box.lo[2], box.scale[2])) << 2);
    keys[i] = (hard << 31) | (octant << 28) | morton;
    index[i] = i;
}

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
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t group = __builtin_amdgcn_readfirstlane(blockIdx.x * kWavesPerGroup + (threadIdx.x >> 6));
    const uint32_t base = group << 6;            // n_pixels <= 2^28 (rtxq::kMaxRays)
    if (base >= n_pixels) return;                // the whole wavefront
    const bool active = base + lane < n_pixels;
    uint32_t pixel = base + lane;
    if (active && order) pixel = order[pixel];
    ShadeTally tally;
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
    if (COUNT && lane == 0 && counters) flush_tally(counters, tally);
}

namespace {

template <bool COUNT, bool SPHERES>
void launch_form(const DeviceScene &S, uint32_t n_pixels, const float *origins, const float *directions, const uint32_t *order,
                 void *out_shade, void *out_hits, unsigned long long *counters, float origin_bound, hipStream_t stream)
{
    const uint32_t groups = (n_pixels + 63u) / 64u;
    const dim3 grid((groups + kWavesPerGroup - 1u) / kWavesPerGroup), block(64u * kWavesPerGroup);
    hipLaunchKernelGGL((shade_kernel<COUNT, SPHERES>), grid, block, 0, stream, S, n_pixels, origins, directions, order,
                       static_cast<uint4 *>(out_shade), static_cast<uint4 *>(out_hits), counters, origin_bound);
}

}  // namespace

hipError_t launch_shade(const DeviceScene &S, uint32_t n_pixels, const float *origins, const float *directions,
                        const rtxq::KeyBox &box, float origin_bound, const rtxq::SortBuffers *sort, void *out_shade,
                        void *out_hits, unsigned long long *counters, hipStream_t stream)
{
    if (n_pixels == 0u) return hipSuccess;
    if (S.nb_ray == 0u || n_pixels > rtxq::kMaxRays / S.nb_ray) return hipErrorInvalidValue;
    const uint32_t *order = nullptr;
    if (sort) {
        hipLaunchKernelGGL(key_kernel, dim3((n_pixels + 255u) / 256u), dim3(256), 0, stream, n_pixels, S.nb_ray, origins,
                           directions, box, sort->keys, sort->index);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
        size_t temp_bytes = sort->temp_bytes;
        e = rocprim::radix_sort_pairs(sort->temp, temp_bytes, sort->keys, sort->keys_sorted, sort->index, sort->index_sorted,
                                      n_pixels, 0u, 32u, stream);
        if (e != hipSuccess) return e;
        order = sort->index_sorted;
    }
    const bool spheres = S.n_spheres != 0u;
    if (counters) {
        if (spheres) launch_form<true, true>(S, n_pixels, origins, directions, order, out_shade, out_hits, counters, origin_bound, stream);
        else launch_form<true, false>(S, n_pixels, origins, directions, order, out_shade, out_hits, counters, origin_bound, stream);
    } else {
        if (spheres) launch_form<false, true>(S, n_pixels, origins, directions, order, out_shade, out_hits, counters, origin_bound, stream);
        else launch_form<false, false>(S, n_pixels, origins, directions, order, out_shade, out_hits, counters, origin_bound, stream);
    }
    return hipGetLastError();
}

}  // namespace rtxs
