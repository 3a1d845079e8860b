// rtx_samples.hip — a scene's seeded sample table made on the device, for gfx950.
//
//   rtx_scene_reseed    the table every later call on the scene reads, made by each device's catch-up
//
// samples_kernel runs scene_prep.h's sample_statement — the text the host compiles too — once per draw.  One work-item
// makes TWO pairs, four draws, and writes them with one 16-byte store: a wavefront writes 1,024 contiguous bytes, the
// widest store a lane has, a quarter of the store instructions of a draw per lane.  A table of an odd number of pairs ends
// in one pair, which the last work-item writes with an 8-byte store.  The statement is 64-bit integer arithmetic (two
// multiplies per draw) and two exact f32 steps; a 2,000,000-pair table is 16 MB written once, so the kernel is bound by the
// stores, not by the arithmetic.  Indices are 64-bit throughout: 2^32 - 1 pairs are 2^33 draws.
//
// No LDS, no atomics, no arrival counters, no spinning; every output word is written by exactly one work-item, and no
// work-item reads what another wrote.  The kernel boundary is the only hand-off: the catch-up that launches it waits for
// it before any reader is enqueued.
//
// The kernel lives in namespace rtxr: librtx.so's other kernel sets stay what they were.
#include "rtx_samples.h"

namespace rtxr {

__global__ void __launch_bounds__(kSamplesBlock) samples_kernel(uint64_t seed, uint64_t n_pairs, float2 *out)
{
    const uint64_t item = static_cast<uint64_t>(blockIdx.x) * kSamplesBlock + threadIdx.x;
    const uint64_t pair = 2ull * item;
    if (pair >= n_pairs) return;
    const uint64_t draw = 2ull * pair;
    const float a = rtx::sample_statement(seed, draw), b = rtx::sample_statement(seed, draw + 1ull);
    if (pair + 1ull < n_pairs) {
        const float c = rtx::sample_statement(seed, draw + 2ull), d = rtx::sample_statement(seed, draw + 3ull);
        *reinterpret_cast<float4 *>(out + pair) = make_float4(a, b, c, d);      // (pair is even, out 16-byte aligned)
    } else {
        out[pair] = make_float2(a, b);
    }
}

hipError_t launch_samples(uint64_t seed, uint32_t n_pairs, float2 *out, hipStream_t stream)
{
    if (n_pairs == 0u) return hipSuccess;
    if (!out || (reinterpret_cast<uintptr_t>(out) & 15u)) return hipErrorInvalidValue;
    const uint64_t items = (static_cast<uint64_t>(n_pairs) + 1ull) / 2ull;              // <= 2^31
    const uint64_t blocks = (items + kSamplesBlock - 1ull) / kSamplesBlock;             // <= 2^23
    hipLaunchKernelGGL(samples_kernel, dim3(static_cast<uint32_t>(blocks)), dim3(kSamplesBlock), 0, stream, seed,
                       static_cast<uint64_t>(n_pairs), out);
    return hipGetLastError();
}

}  // namespace rtxr
