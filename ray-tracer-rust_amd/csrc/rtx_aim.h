// rtx_aim.h — the launcher of the aim kernels (rtx_aim.hip), shared with rtx_api.cpp.
//
// rtx_render_view_rows (include/rtx.h) renders any pinhole view of an uploaded scene through the render pipeline.  The
// pipeline's primary rays walk a stream that puts, of every node's two children, the one nearer the EYE first
// (PreparedScene::primary_nodes, scene_prep.cpp: stream_nearest_first); a view with another eye gets that stream made on
// the device, from the shadow stream as it is uploaded.  The kernels live in a namespace of their own, rtxa, beside the
// render pipeline's (rtx), the ray queries' (rtxq), ray shading's (rtxs) and the view kernels' (rtxv), whose kernel sets
// stay what they were.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "scene_prep.h"

namespace rtxa {

// what pass 1 leaves for pass 2, one per record: the record's parent and the size (in records) of the sibling that is
// visited ahead of it, 0 for the child visited first
struct AimLink {
    uint32_t parent, before;
};
static_assert(sizeof(AimLink) == 8, "one 8-byte store per record");

// stream_nearest_first's child order of two boxes as the device holds them (planes moved by cull_delta): the first child
// stays first unless the second one's centre is nearer `eye`.  Every operation in double, rounded once, in this order —
// host (rtx_scene_aimed_nodes goes through scene_prep.cpp's dist2, the same expression) and device agree bit for bit.
// nodes: the uploaded shadow stream, n_nodes records; out: n_nodes records (the caller keeps a zeroed sentinel behind
// them); links: n_nodes entries of scratch.  root: first record of the tree proper; records before it are copied.
// Two launches on `stream`; n_nodes == 0: nothing.
hipError_t launch_aim(const rtx::NodeDev *nodes, uint32_t n_nodes, uint32_t root, const float eye[3], AimLink *links,
                      rtx::NodeDev *out, hipStream_t stream);

}  // namespace rtxa
