// rtx_planes.h — the launcher of the plane kernel (rtx_planes.hip), shared with rtx_api.cpp.
//
// rtx_render_view_rows_posed (include/rtx.h) renders a pose through the render pipeline.  The pipeline's shading pass
// certifies "this ray cannot hit the first global triangle" from that triangle's plane record alone (rtx_traverse.hpp:
// plane_rules_out) and then leaves the triangle out of the walk, so a pose needs the records of ITS global triangles: a stale
// one is a wrong frame, not a slow one.  A pose makes them with its records, on its stream, from the statement the host
// compiles too (scene_prep.h: global_plane_statement).  The kernel lives in a namespace of its own, rtxg, beside rtx, rtxq,
// rtxs, rtxv, rtxa, rtxl, rtxt and rtxp, whose kernel sets stay what they were.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "scene_prep.h"

namespace rtxg {

// rtx::global_plane_statement over posed primitive records [0, n_global) (leaf order: the global triangles come first),
// word for word the host's: one work-item per record, 16 words each into `out`.  On `stream`, behind the kernel that makes
// the records; nothing is waited for.  n_global == 0: nothing is launched.
hipError_t launch_global_planes(const rtx::TriRec *tris, uint32_t n_global, rtx::TriRec *out, hipStream_t stream);

}  // namespace rtxg
