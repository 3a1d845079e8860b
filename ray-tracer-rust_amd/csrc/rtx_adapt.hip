// rtx_adapt.hip — the adaptive mean of N frames: tiles stop once their noise estimate is met, for gfx950.
//
//   rtx_render_view_adaptive     per frame view_masked_kernel then moment_add_kernel, moment_resolve_kernel after the last frame
//   rtx_moment_add_device        moment_add_kernel over a caller's records
//   rtx_moment_resolve_device    moment_resolve_kernel over a caller's moments
//
// view_masked_kernel: rtxv::view_kernel's tile body behind one wave-uniform test.  The body is RESTATED here (view_tile,
// records only): lifted into a header as a forced-inline function of the tile number, every form tried — arguments by
// reference or by value, with and without __restrict__ — changed rtxv::view_kernel's schedule and register allocation
// (tools/same_isa.py: DIFF for its four forms), so rtx_view.hip stays untouched.  The wavefront
// computes its tile number, leaves if it is past the launch's tiles and then, unless `first`, reads the tile's 8-byte state
// and leaves when tile_stopped (scene_prep.h) says so.  The state's two words are made scalars (v_readfirstlane): the test
// is a scalar branch in front of a body that votes and reads lanes.  It writes RtxPixelShade records only.
//
// moment_add_kernel: one wavefront per tile of the rectangle, lane l pixel (8tx + (l & 7), 8ty + (l >> 3)) as in the view
// kernel, four independent wavefronts per workgroup.  The same test first: a stopped tile's moments and state are not
// touched.  A lane inside the rectangle then loads its record (16 bytes) and its moments (two 16-byte loads, skipped under
// `first`), runs moment_add_statement, stores the moments (two 16-byte stores) and runs moment_error_statement; lanes
// outside load and store nothing and contribute +0.0.  The wavefront's maximum is a six-step butterfly of cross-lane reads
// (no LDS): every value is >= 0 and none is a NaN, so its shape does not matter.  Lane 0 writes the state {frames, err}
// with one ordinary 8-byte store.  A wavefront touches eight runs of 128 bytes of records and of 256 bytes of moments.
//
// moment_resolve_kernel: rtxc::accum_resolve_kernel's shape — the scene's 256 thresholds staged in LDS once per
// workgroup, one pixel per work-item, two 16-byte loads, an optional 16-byte record store and an optional RGB8 store of
// three byte stores, so out_rgb may have any alignment.  The divisor is the pixel's own frame count.
//
// No atomics, no arrival counters, no spinning; every output word has exactly one writer.  The tile state a wavefront reads
// was written by an earlier launch: the kernel boundary is the only hand-off.
//
// The kernels live in namespace rtxe: librtx.so's other kernel sets stay what they were.
#include "rtx_adapt.h"
#include "rtx_shade_pixel.hpp"

namespace rtxe {

using namespace rtx;

namespace {

// the tile's state as two scalars
__device__ __forceinline__ RtxTileState tile_state(const RtxTileState *tiles, uint32_t tile)
{
    const uint2 w = *reinterpret_cast<const uint2 *>(tiles + tile);
    RtxTileState st;
    st.frames = __builtin_amdgcn_readfirstlane(w.x);
    st.err = __uint_as_float(__builtin_amdgcn_readfirstlane(w.y));
    return st;
}

// rtxv::view_kernel's body (rtx_view.hip) for tile `tile` of the rectangle, writing records only: lane l is pixel
// (x0 + 8*tx + (l & 7), y0 + 8*ty + (l >> 3)); the rays are made in registers from the view block with create_rays'
// arithmetic; the per-ray body is rtx_shade_pixel.hpp's shade_ray.  Lanes outside the rectangle carry a harmless regular ray
// and never vote.
template <bool COUNT, bool SPHERES>
__device__ __forceinline__ void view_tile(const DeviceScene &S, const rtxv::ViewBlock &V, uint32_t tiles_x, uint32_t tile, uint32_t lane,
                                          uint4 *__restrict__ out_shade, unsigned long long *__restrict__ counters,
                                          float origin_bound, uint32_t eye_in_range)
{
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
                                  active ? rz : 1.0f, eye_in_range != 0u, origin_bound, denom, nullptr, slot * S.nb_ray + k,
                                  sum, tally);
    }
    if (active) out_shade[slot] = pixel_word(sum, pixel_bytes(S, sum));
    if (COUNT) flush_tally(counters, lane, tally);
}

}  // namespace

template <bool COUNT, bool SPHERES>
__global__ void __launch_bounds__(64 * kWavesPerGroup) view_masked_kernel(DeviceScene S, rtxv::ViewBlock V, uint32_t tiles_x,
                                                                          uint32_t n_tiles, uint4 *__restrict__ out_shade,
                                                                          unsigned long long *__restrict__ counters,
                                                                          float origin_bound, uint32_t eye_in_range,
                                                                          const RtxTileState *__restrict__ tiles, uint32_t first,
                                                                          RtxAdaptRule rule)
{
    uint32_t lane;
    const uint32_t tile = wave_of_launch(lane);
    if (tile >= n_tiles) return;                 // the whole wavefront
    if (!first && tile_stopped(rule, tile_state(tiles, tile))) return;               // ... and again
    view_tile<COUNT, SPHERES>(S, V, tiles_x, tile, lane, out_shade, counters, origin_bound, eye_in_range);
}

__global__ void __launch_bounds__(64 * kWavesPerGroup) moment_add_kernel(uint32_t nx, uint32_t ny, uint32_t tiles_x, uint32_t n_tiles,
                                                                         uint32_t first, RtxAdaptRule rule,
                                                                         const uint4 *__restrict__ shade, uint4 *__restrict__ moments,
                                                                         RtxTileState *tiles)
{
    uint32_t lane;
    const uint32_t tile = wave_of_launch(lane);
    if (tile >= n_tiles) return;                 // the whole wavefront
    uint32_t frames = 0u;
    if (tiles && !first) {
        const RtxTileState st = tile_state(tiles, tile);
        if (tile_stopped(rule, st)) return;      // the whole wavefront: nothing of the tile is touched
        frames = st.frames;
    }
    const uint32_t ty = tile / tiles_x, tx = tile - ty * tiles_x;
    const uint32_t lx = tx * 8u + (lane & 7u), ly = ty * 8u + (lane >> 3);
    float err = 0.0f;
    if (lx < nx && ly < ny) {
        const size_t slot = (size_t)ly * nx + lx;                                    // < 2^28
        const uint4 in = shade[slot];
        RtxPixelShade s;
        __builtin_memcpy(&s, &in, sizeof s);
        uint4 words[2] = {{0u, 0u, 0u, 0u}, {0u, 0u, 0u, 0u}};
        if (!first) {
            words[0] = moments[2u * slot];
            words[1] = moments[2u * slot + 1u];
        }
        RtxMomentPixel m;
        __builtin_memcpy(&m, words, sizeof m);
        moment_add_statement(first != 0u, s, &m);
        __builtin_memcpy(words, &m, sizeof m);
        moments[2u * slot] = words[0];
        moments[2u * slot + 1u] = words[1];
        err = moment_error_statement(m);
    }
    for (int step = 32; step; step >>= 1) {
        const float other = __shfl_xor(err, step, 64);
        err = err < other ? other : err;
    }
    if (tiles && lane == 0u) {
        RtxTileState st;
        st.frames = frames + 1u;
        st.err = err;
        tiles[tile] = st;
    }
}

__global__ void __launch_bounds__(kResolveBlock) moment_resolve_kernel(const float *__restrict__ thr, uint32_t n,
                                                                       const uint4 *__restrict__ moments,
                                                                       uint8_t *__restrict__ out_rgb, uint4 *__restrict__ out_shade)
{
    static_assert(kResolveBlock == 256u, "one threshold per work-item");
    __shared__ float l_thr[256];
    l_thr[threadIdx.x] = thr[threadIdx.x];
    __syncthreads();
    const uint32_t pixel = blockIdx.x * kResolveBlock + threadIdx.x;
    if (pixel >= n) return;
    const uint4 words[2] = {moments[2ull * pixel], moments[2ull * pixel + 1u]};
    RtxMomentPixel m;
    __builtin_memcpy(&m, words, sizeof m);
    const RtxPixelShade s = moment_resolve_statement(l_thr, m);
    if (out_shade) {
        uint4 out;
        __builtin_memcpy(&out, &s, sizeof out);
        out_shade[pixel] = out;
    }
    if (out_rgb) {
        uint8_t *p = out_rgb + 3ull * pixel;
        p[0] = s.rgb8[0];
        p[1] = s.rgb8[1];
        p[2] = s.rgb8[2];
    }
}

hipError_t launch_view_masked(const DeviceScene &S, const rtxv::ViewBlock &V, float origin_bound, void *d_shade,
                              unsigned long long *counters, const void *d_tiles, bool first, const RtxAdaptRule &rule,
                              hipStream_t stream)
{
    if (V.nx == 0u || V.ny == 0u) return hipSuccess;
    const uint64_t rays = static_cast<uint64_t>(V.nx) * V.ny * S.nb_ray;
    if (S.nb_ray == 0u || S.n_samples == 0u || rays > rtxv::kMaxRays) return hipErrorInvalidValue;
    if (!d_shade || (reinterpret_cast<uintptr_t>(d_shade) & 15u) || (!d_tiles && !first) || (reinterpret_cast<uintptr_t>(d_tiles) & 7u))
        return hipErrorInvalidValue;
    const uint64_t tiles_x = (static_cast<uint64_t>(V.nx) + 7u) / 8u, n_tiles = tile_count(V.nx, V.ny);
    if (n_tiles > 0x7FFFFFFFull) return hipErrorInvalidValue;
    // origins_in_range (rtx_ray_walk.hpp) for the one origin every lane has
    const bool eye_in_range = fabsf(V.eye[0]) <= origin_bound && fabsf(V.eye[1]) <= origin_bound && fabsf(V.eye[2]) <= origin_bound;
    launch_form(counters != nullptr, S.n_spheres != 0u, static_cast<uint32_t>(n_tiles), [&](auto count, auto spheres, dim3 grid, dim3 block) {
        hipLaunchKernelGGL((view_masked_kernel<count.value, spheres.value>), grid, block, 0, stream, S, V, static_cast<uint32_t>(tiles_x),
                           static_cast<uint32_t>(n_tiles), static_cast<uint4 *>(d_shade), counters, origin_bound,
                           eye_in_range ? 1u : 0u, static_cast<const RtxTileState *>(d_tiles), first ? 1u : 0u, rule);
    });
    return hipGetLastError();
}

hipError_t launch_moment_add(uint32_t nx, uint32_t ny, const void *shade, void *moments, void *tiles, bool first,
                             const RtxAdaptRule &rule, hipStream_t stream)
{
    if (nx == 0u || ny == 0u) return hipSuccess;
    if (!shade || !moments || ((reinterpret_cast<uintptr_t>(shade) | reinterpret_cast<uintptr_t>(moments)) & 15u) ||
        (reinterpret_cast<uintptr_t>(tiles) & 7u))
        return hipErrorInvalidValue;
    if (static_cast<uint64_t>(nx) * ny > kMaxPixels) return hipErrorInvalidValue;
    const uint64_t tiles_x = (static_cast<uint64_t>(nx) + 7u) / 8u, n_tiles = tile_count(nx, ny);
    if (n_tiles > 0x7FFFFFFFull) return hipErrorInvalidValue;
    const uint32_t groups = static_cast<uint32_t>((n_tiles + kWavesPerGroup - 1u) / kWavesPerGroup);
    hipLaunchKernelGGL(moment_add_kernel, dim3(groups), dim3(64u * kWavesPerGroup), 0, stream, nx, ny, static_cast<uint32_t>(tiles_x),
                       static_cast<uint32_t>(n_tiles), first ? 1u : 0u, tiles ? rule : RtxAdaptRule{1u, 0.0f},
                       static_cast<const uint4 *>(shade), static_cast<uint4 *>(moments), static_cast<RtxTileState *>(tiles));
    return hipGetLastError();
}

hipError_t launch_moment_resolve(const float *thr, uint32_t n, const void *moments, void *out_rgb, void *out_shade,
                                 hipStream_t stream)
{
    if (n == 0u) return hipSuccess;
    if (!thr || !moments || (!out_rgb && !out_shade)) return hipErrorInvalidValue;
    if ((reinterpret_cast<uintptr_t>(moments) | reinterpret_cast<uintptr_t>(out_shade)) & 15u) return hipErrorInvalidValue;
    const uint32_t blocks = static_cast<uint32_t>((static_cast<uint64_t>(n) + kResolveBlock - 1u) / kResolveBlock);
    hipLaunchKernelGGL(moment_resolve_kernel, dim3(blocks), dim3(kResolveBlock), 0, stream, thr, n,
                       static_cast<const uint4 *>(moments), static_cast<uint8_t *>(out_rgb), static_cast<uint4 *>(out_shade));
    return hipGetLastError();
}

}  // namespace rtxe
