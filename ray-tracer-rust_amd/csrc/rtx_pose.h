// rtx_pose.h — the launchers of the pose kernels (rtx_pose.hip), shared with rtx_api.cpp.
//
// rtx_scene_pose and rtx_scene_pose_device (include/rtx.h) move the triangles of an uploaded scene.  The ray-batch kernels
// read geometry through S.nodes, S.tris, S.shade, S.ref_nodes / S.n_ref_nodes and S.n_global alone (rtx_ray_walk.hpp), so a
// posed call is its unposed twin with those pointers of its DeviceScene copy swapped; what it needs made is the posed
// primitive and shading records and the refitted node stream, on the device, on the call's stream.  The statement both
// sides compile is scene_prep.h's (triangle_statement, PoseTables, posed_records).  The kernels live in a namespace of
// their own, rtxp, beside rtx, rtxq, rtxs, rtxv, rtxa, rtxl and rtxt, whose kernel sets stay what they were.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "scene_prep.h"

namespace rtxp {

// the uploaded scene (read only), the host tables (rtx::PoseTables, uploaded once per scene and device) and the pose's
// buffers (library-owned, written by the kernels)
struct PoseArgs {
    const rtx::TriRec *tris;          // n_prims uploaded records, leaf order
    const rtx::ShadeRec *shade;       // n_prims, Vec order
    const rtx::NodeDev *nodes;        // n_nodes uploaded records: link and info are taken from them
    const uint32_t *tri_of;           // n_prims
    const uint2 *ranges;              // n_nodes x {first, count}
    const uint32_t *order;            // n_nodes: the n_long long ranges first
    uint32_t n_prims, n_nodes, n_long;
    float cull_delta;                 // the scene's
    const float *pose;                // n_tris x 9, the caller's
    const uint32_t *rank;             // n_prims per Vec position, or NULL: the position
    rtx::TriRec *out_tris;            // n_prims
    rtx::ShadeRec *out_shade;         // n_prims
    rtx::NodeDev *out_nodes;          // n_nodes
};

// rtx::posed_records on the device, word for word: one launch for the primitive and shading records (one work-item per
// record), then the refit, which reads what that launch wrote: one launch for the ranges of more than rtx::kPoseLaneMax
// records (one workgroup of rtx::kPoseBlock per node) and one for the others (one work-item per node).  No work-item reads
// a box another workgroup wrote in the same launch.  All on `stream`; nothing is waited for.
hipError_t launch_pose(const PoseArgs &a, hipStream_t stream);
// The refit alone, over records something else has put into out_tris on `stream` (rtx_rebuild.hip: a rebuilt pose's sorted
// records): nodes, ranges, order, n_long and n_nodes are then the rebuilt stream's tables.  Reads nodes (link and info),
// ranges, order and out_tris; writes out_nodes.
hipError_t launch_refit(const PoseArgs &a, hipStream_t stream);

}  // namespace rtxp
