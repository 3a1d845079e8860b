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
// The walks are rtx_traverse.hpp's, chosen as the ray-query kernels choose them (rtx_query.hip): closest_hit for the
// primary ray, any_hit with limit = distance to the light point for a shadow ray; a 64-lane walk holding a "hard"
// direction goes through closest_hit_reference; a walk holding an origin beyond origin_bound uses the exact slab test.
// That last vote is taken twice: on the caller's origins for the primary walk and on the HIT POINTS for the shadow walks
// (a far origin's p_hit can round to just outside the bound although the scene lies inside it).
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
#include "rtx_traverse.hpp"

namespace rtxs {

using namespace rtx;

namespace {

constexpr uint32_t kWavesPerGroup = 4u;      // independent wavefronts: no barrier, no LDS
constexpr uint32_t kNoHit = 0xFFFFFFFFu;     // RTX_NO_HIT

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
__device__ __forceinline__ uint32_t quantise(const float *__restrict__ thr, float x)
{
    uint32_t b = 0;
#pragma unroll
    for (uint32_t step = 128; step; step >>= 1)
        if (x >= thr[b + step]) b += step;
    return b;
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
    const TriRec RTX_CONSTANT *tris = (const TriRec RTX_CONSTANT *)S.tris;
    const NodeRec RTX_CONSTANT *nodes = (const NodeRec RTX_CONSTANT *)S.nodes;
    const float RTX_CONSTANT *lights = (const float RTX_CONSTANT *)S.light_points;   // wave-uniform reads: scalar operands
    WaveCounters wc;
    unsigned long long primary_hits = 0, reference_walks = 0;
    float acc_r = 0.0f, acc_g = 0.0f, acc_b = 0.0f;                                  // avg_col, main.rs:182
    uint32_t n_hit = 0;
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
        float hx = 0.0f, hy = 0.0f, hz = 0.0f, nx = 0.0f, ny = 0.0f, nz = 0.0f, cr = 0.0f, cg = 0.0f, cb = 0.0f;
        bool hit;
        {
            float len, dx, dy, dz;
            (void)length_and_direction(vx, vy, vz, len, dx, dy, dz);
            LaneRay r = make_ray(active, ox, oy, oz, dx, dy, dz);
            const bool walked = origins_in_range(active, ox, oy, oz, origin_bound)
                                    ? closest_hit<COUNT, true, SPHERES>(nodes, tris, S.shade, S.n_nodes, r, wc, S.n_global)
                                    : closest_hit<COUNT, false, SPHERES>(nodes, tris, S.shade, S.n_nodes, r, wc, S.n_global);
            if (!walked) {
                uint32_t n_stream;
                bool have_ref;
                const NodeRec RTX_CONSTANT *stream = reference_stream(S, n_stream, have_ref);
                closest_hit_reference<COUNT, SPHERES>(stream, tris, S.shade, n_stream, have_ref, active, ox, oy, oz, dx, dy, dz,
                                                      r.best_t, r.best_idx, wc);
                reference_walks += 1;
            }
            hit = active && r.best_idx != kNone;
            uint4 w0 = make_uint4(kNoHit, 0u, 0u, 0u), w1 = make_uint4(0u, 0u, 0u, 0u);
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
                out_hits[2u * ray] = w0;
                out_hits[2u * ray + 1u] = w1;
            }
        }
        const unsigned long long hit_mask = ballot(hit);
        if (hit_mask == 0ull) continue;                                              // main.rs:188: every lane's `None` arm
        if (COUNT) primary_hits += __popcll(hit_mask);
        if (hit && n_hit < 255u) ++n_hit;
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
                reference_walks += 1;
            }
            const float lnd = fabsf(nx * dx + ny * dy + nz * dz);                    // main.rs:207
            // an occluded sample adds (black * 1.0) / denom = +0.0 (main.rs:226): left out, as shade_tiles_kernel leaves it out
            if (hit && !occluded) {
                acc_r = acc_r + ((cr * lnd) / denom);                                // main.rs:211-215
                acc_g = acc_g + ((cg * lnd) / denom);
                acc_b = acc_b + ((cb * lnd) / denom);
            }
        }
    }
    if (active) {
        const uint32_t bytes = quantise(S.gamma_thr, acc_r) | (quantise(S.gamma_thr, acc_g) << 8) |
                               (quantise(S.gamma_thr, acc_b) << 16) | (n_hit << 24);
        out_shade[pixel] = make_uint4(__float_as_uint(acc_r), __float_as_uint(acc_g), __float_as_uint(acc_b), bytes);
    }
    if (COUNT && lane == 0 && counters) {
        if (primary_hits) atomicAdd(&counters[0], primary_hits);
        atomicAdd(&counters[1], wc.box_tests);
        atomicAdd(&counters[2], wc.tri_tests);
        atomicAdd(&counters[3], wc.node_visits);
        atomicAdd(&counters[4], wc.tri_visits);
        if (reference_walks) atomicAdd(&counters[5], reference_walks);
    }
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
