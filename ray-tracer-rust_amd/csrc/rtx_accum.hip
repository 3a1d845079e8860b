// rtx_accum.hip — the mean of N frames kept on the device, for gfx950.
//
//   rtx_render_view_mean         per frame accum_add_kernel behind the view kernel, accum_resolve_kernel after the last frame
//   rtx_accum_add_device         accum_add_kernel over a caller's records
//   rtx_accum_resolve_device     accum_resolve_kernel over a caller's accumulator
//
// Both kernels run scene_prep.h's statements — the text the host compiles too — once per pixel, and both are bound by the
// bytes they move: an add reads 16 + 16 bytes (16 under `first`) and writes 16 per pixel with two additions per channel
// word, a resolve reads 16 and writes up to 16 + 3 with three divisions and 24 LDS reads.
//
// accum_add_kernel: one record per work-item — one 16-byte load of the frame's record, one of the accumulator (skipped
// under `first`, a launch-uniform argument: the old content may be anything), one 16-byte store.  A wavefront touches 1,024
// contiguous bytes of each array.
//
// accum_resolve_kernel: the scene's 256 thresholds are staged in LDS once per workgroup (one word per work-item), since the
// search is eight DEPENDENT reads per channel at addresses that differ from lane to lane, as in shade_tiles_kernel.  A
// work-item then takes ONE pixel: one 16-byte load, an optional 16-byte record store — a wavefront touches 1,024 contiguous
// bytes of each — and an optional RGB8 store of three byte stores, so out_rgb may have any alignment and no byte outside
// [out_rgb, out_rgb + 3n) is written.  A form in which a work-item took four pixels and wrote their twelve bytes as three
// dwords (byte stores for the unaligned head and the tail) was measured beside this one and is not kept: its 16-byte loads
// and stores lie 64 bytes apart from lane to lane, and it took 2.7 times as long with the records written and 7 % longer
// with RGB8 alone.
//
// No atomics, no arrival counters, no spinning; every output word has exactly one writer, and no work-item reads what
// another wrote but the staged thresholds, behind the workgroup's one barrier.  The kernel boundary is the only hand-off.
//
// The kernels live in namespace rtxc: librtx.so's other kernel sets stay what they were.
#include "rtx_accum.h"

namespace rtxc {

namespace {

__device__ __forceinline__ RtxPixelShade resolve_pixel(const float *thr, uint32_t n_frames, const uint4 *__restrict__ accum,
                                                       uint4 *__restrict__ out_shade, uint32_t pixel)
{
    const uint4 words = accum[pixel];
    RtxAccumPixel a;
    __builtin_memcpy(&a, &words, sizeof a);
    const RtxPixelShade s = rtx::accum_resolve_statement(thr, n_frames, a);
    if (out_shade) {
        uint4 out;
        __builtin_memcpy(&out, &s, sizeof out);
        out_shade[pixel] = out;
    }
    return s;
}

}  // namespace

__global__ void __launch_bounds__(kAccumBlock) accum_add_kernel(uint32_t n, uint32_t first, const uint4 *__restrict__ shade,
                                                                uint4 *__restrict__ accum)
{
    const uint32_t i = blockIdx.x * kAccumBlock + threadIdx.x;
    if (i >= n) return;
    const uint4 in = shade[i];
    RtxPixelShade s;
    __builtin_memcpy(&s, &in, sizeof s);
    RtxAccumPixel a = {{0.0f, 0.0f, 0.0f}, 0u};
    if (!first) {
        const uint4 old = accum[i];
        __builtin_memcpy(&a, &old, sizeof a);
    }
    rtx::accum_add_statement(first != 0u, s, &a);
    uint4 out;
    __builtin_memcpy(&out, &a, sizeof out);
    accum[i] = out;
}

__global__ void __launch_bounds__(kAccumBlock) accum_resolve_kernel(const float *__restrict__ thr, uint32_t n, uint32_t n_frames,
                                                                    const uint4 *__restrict__ accum, uint8_t *__restrict__ out_rgb,
                                                                    uint4 *__restrict__ out_shade)
{
    static_assert(kAccumBlock == 256u, "one threshold per work-item");
    __shared__ float l_thr[256];
    l_thr[threadIdx.x] = thr[threadIdx.x];
    __syncthreads();
    const uint32_t pixel = blockIdx.x * kAccumBlock + threadIdx.x;
    if (pixel >= n) return;
    const RtxPixelShade s = resolve_pixel(l_thr, n_frames, accum, out_shade, pixel);
    if (out_rgb) {
        uint8_t *p = out_rgb + 3ull * pixel;
        p[0] = s.rgb8[0];
        p[1] = s.rgb8[1];
        p[2] = s.rgb8[2];
    }
}

hipError_t launch_accum_add(uint32_t n, const void *shade, void *accum, bool first, hipStream_t stream)
{
    if (n == 0u) return hipSuccess;
    if (!shade || !accum || ((reinterpret_cast<uintptr_t>(shade) | reinterpret_cast<uintptr_t>(accum)) & 15u)) return hipErrorInvalidValue;
    const uint32_t blocks = static_cast<uint32_t>((static_cast<uint64_t>(n) + kAccumBlock - 1u) / kAccumBlock);
    hipLaunchKernelGGL(accum_add_kernel, dim3(blocks), dim3(kAccumBlock), 0, stream, n, first ? 1u : 0u,
                       static_cast<const uint4 *>(shade), static_cast<uint4 *>(accum));
    return hipGetLastError();
}

hipError_t launch_accum_resolve(const float *thr, uint32_t n, const void *accum, uint32_t n_frames, void *out_rgb,
                                void *out_shade, hipStream_t stream)
{
    if (n == 0u) return hipSuccess;
    if (!thr || !accum || (!out_rgb && !out_shade) || n_frames == 0u || n_frames > rtx::kMaxMeanFrames) return hipErrorInvalidValue;
    if ((reinterpret_cast<uintptr_t>(accum) | reinterpret_cast<uintptr_t>(out_shade)) & 15u) return hipErrorInvalidValue;
    const uint32_t blocks = static_cast<uint32_t>((static_cast<uint64_t>(n) + kAccumBlock - 1u) / kAccumBlock);
    hipLaunchKernelGGL(accum_resolve_kernel, dim3(blocks), dim3(kAccumBlock), 0, stream, thr, n, n_frames,
                       static_cast<const uint4 *>(accum), static_cast<uint8_t *>(out_rgb), static_cast<uint4 *>(out_shade));
    return hipGetLastError();
}

}  // namespace rtxc
