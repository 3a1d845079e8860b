// rtx_adapt.h — the launchers of the adaptive mean's kernels (rtx_adapt.hip), shared with rtx_api.cpp.
//
// rtx_render_view_adaptive (include/rtx.h) averages up to N frames of a view on the device and stops rendering an 8 x 8
// tile once its noise estimate is met: every frame's RtxPixelShade records are added into an array of RtxMomentPixel (sum,
// sum of squares, the pixel's own frame count), the add leaves an RtxTileState {frames, err} per tile, and the next frame's
// view launch and add return at once for the tiles that tile_stopped(rule, state) names.  All of it is scene_prep.h's
// statements (moment_add_statement, moment_error_statement, tile_stopped, moment_resolve_statement), the text the host
// compiles too.  The kernels live in a namespace of their own, rtxe, beside rtx, rtxq, rtxs, rtxv, rtxa, rtxl, rtxt, rtxp,
// rtxg, rtxb, rtxm, rtxf, rtxk, rtxr and rtxc, whose kernel sets stay what they were.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "rtx_view.h"
#include "scene_prep.h"

namespace rtxe {

constexpr uint32_t kResolveBlock = 256u;
constexpr uint64_t kMaxPixels = 1ull << 28;      // records of one rectangle (rtxv::kMaxRays at one ray per pixel)

// the tiles of an nx x ny rectangle, row by row: ceil(nx/8) * ceil(ny/8)
inline uint64_t tile_count(uint32_t nx, uint32_t ny) { return ((static_cast<uint64_t>(nx) + 7u) / 8u) * ((static_cast<uint64_t>(ny) + 7u) / 8u); }

// rtxv::launch_view's records (d_shade: nx*ny RtxPixelShade, 16-byte aligned, never NULL) for the tiles that are live:
// every tile under `first` (d_tiles is not read), otherwise the tiles with !tile_stopped(rule, d_tiles[tile]).  The records
// of a stopped tile are not written.  d_tiles: tile_count() RtxTileState, 8-byte aligned, may be NULL only under `first`
// (else hipErrorInvalidValue).  Everything else as rtxv::launch_view.
hipError_t launch_view_masked(const rtx::DeviceScene &S, const rtxv::ViewBlock &V, float origin_bound, void *d_shade,
                              unsigned long long *counters, const void *d_tiles, bool first, const RtxAdaptRule &rule,
                              hipStream_t stream);

// For every live tile of the nx x ny rectangle: moments[p] = moment_add_statement(first, shade[p], moments[p]) for its
// pixels p = y * nx + x inside the rectangle, and tiles[tile] = {frames + 1 (1 under first), the maximum of
// moment_error_statement over those pixels}.  A stopped tile's moments and state are not touched.  tiles == NULL: every tile
// is live, no state is written, rule is not read.  shade, moments 16-byte and tiles 8-byte aligned, nx * ny <= kMaxPixels
// (else hipErrorInvalidValue).  One launch on `stream`; an empty rectangle: nothing.
hipError_t launch_moment_add(uint32_t nx, uint32_t ny, const void *shade, void *moments, void *tiles, bool first,
                             const RtxAdaptRule &rule, hipStream_t stream);

// record i of out_shade, bytes [3i, 3i + 3) of out_rgb = moment_resolve_statement(thr, moments[i]) for i < n.  thr: the
// scene's 256 thresholds on the device; moments and out_shade (NULL or n records) 16-byte aligned; out_rgb NULL or n * 3
// bytes at ANY address; not both NULL (else hipErrorInvalidValue).  One launch; n == 0: nothing.
hipError_t launch_moment_resolve(const float *thr, uint32_t n, const void *moments, void *out_rgb, void *out_shade,
                                 hipStream_t stream);

}  // namespace rtxe
