// rtx_samples.h — the launcher of the sample-table kernel (rtx_samples.hip), shared with rtx_api.cpp.
//
// rtx_scene_reseed (include/rtx.h) replaces a scene's sample table by the seeded one, rtxh_gen_samples(seed, n_pairs) word
// for word.  Every draw of that table is a closed form of (seed, index) — scene_prep.h's sample_statement, the text the host
// compiles too — so a device makes its copy from 12 bytes of input and nothing of the table's size crosses the bus.  The
// kernel lives in a namespace of its own, rtxr, beside rtx, rtxq, rtxs, rtxv, rtxa, rtxl, rtxt, rtxp, rtxg, rtxb, rtxm, rtxf
// and rtxk, whose kernel sets stay what they were.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "scene_prep.h"

namespace rtxr {

constexpr uint32_t kSamplesBlock = 256u;

// out[k] = (sample_statement(seed, 2k), sample_statement(seed, 2k + 1)) for k < n_pairs: the table the pipeline, the view,
// shade and light kernels read as const float2 *.  out: library-owned, 16-byte aligned, at least n_pairs x 8 bytes.  One
// launch; every word has one writer and no work-item reads what another wrote.  On `stream`; nothing is waited for.
hipError_t launch_samples(uint64_t seed, uint32_t n_pairs, float2 *out, hipStream_t stream);

}  // namespace rtxr
