// rtx_accum.h — the launchers of the accumulator kernels (rtx_accum.hip), shared with rtx_api.cpp.
//
// rtx_render_view_mean (include/rtx.h) averages N frames of a view on the device: every frame's RtxPixelShade records are
// added into an array of RtxAccumPixel, and the sums are resolved once — divided, quantised through the scene's gamma
// thresholds — into the records and the bytes a single frame's call gives.  rtx_accum_add_device and
// rtx_accum_resolve_device hand a caller the two steps for frames of its own.  Both steps are scene_prep.h's statements
// (accum_add_statement, accum_resolve_statement), the text the host compiles too.  The kernels live in a namespace of their
// own, rtxc, beside rtx, rtxq, rtxs, rtxv, rtxa, rtxl, rtxt, rtxp, rtxg, rtxb, rtxm, rtxf, rtxk and rtxr, whose kernel sets
// stay what they were.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "scene_prep.h"

namespace rtxc {

constexpr uint32_t kAccumBlock = 256u;

// accum[i] = accum_add_statement(first, shade[i], accum[i]) for i < n.  shade: n RtxPixelShade, accum: n RtxAccumPixel, both
// 16-byte aligned (else hipErrorInvalidValue).  first: accum is written, never read.  One launch on `stream`; n == 0: nothing.
hipError_t launch_accum_add(uint32_t n, const void *shade, void *accum, bool first, hipStream_t stream);

// record i of out_shade, bytes [3i, 3i + 3) of out_rgb = accum_resolve_statement(thr, n_frames, accum[i]) for i < n.  thr: the
// scene's 256 thresholds on the device; accum and out_shade (NULL or n records) 16-byte aligned; out_rgb NULL or n * 3 bytes
// at ANY address; not both NULL; 1 <= n_frames <= rtx::kMaxMeanFrames (else hipErrorInvalidValue).  One launch; n == 0: nothing.
hipError_t launch_accum_resolve(const float *thr, uint32_t n, const void *accum, uint32_t n_frames, void *out_rgb,
                                void *out_shade, hipStream_t stream);

}  // namespace rtxc
