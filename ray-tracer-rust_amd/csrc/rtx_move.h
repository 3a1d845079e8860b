// rtx_move.h — the launcher of the move kernel (rtx_move.hip), shared with rtx_api.cpp.
//
// rtx_scene_pose_moved and rtx_scene_pose_moved_device (include/rtx.h) make a pose's vertices and spheres on the device:
// the scene's geometry as created (the "rest" geometry, uploaded once per scene and device) under a small set of affine
// maps, one named per primitive.  The kernel writes the two arrays rtx_scene_pose_prims_device is handed as v0v1v2 and
// spheres, and everything behind it — the overlay, the pose or rebuild kernels, the refit, the plane records — runs as
// for any pose.  The statement both sides compile is scene_prep.h's move_statement.  The kernel lives in a namespace of
// its own, rtxf, beside rtx, rtxq, rtxs, rtxv, rtxa, rtxl, rtxt, rtxp, rtxg, rtxb and rtxm, whose kernel sets stay what
// they were.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "scene_prep.h"

namespace rtxf {

constexpr uint32_t kMoveBlock = 256u;

// the rest geometry and its tables (read only, library-owned), the call's arrays and the two output buffers
// (library-owned, written by the kernel)
struct MoveArgs {
    const float *rest_v;              // n_triangles x 9
    const float *rest_spheres;        // n_spheres x 4
    const uint32_t *tri_vec;          // n_triangles: triangle number -> Vec position (read when group is given)
    const uint32_t *sphere_vec;       // n_spheres: sphere number -> Vec position (read when group is given)
    uint32_t n_triangles, n_spheres;
    uint32_t n_moves;
    const float *moves;               // n_moves x 12
    const uint32_t *group;            // NULL (every primitive follows move 0) or one per Vec position
    const float *radius_scale;        // NULL or n_moves
    float *out_v;                     // n_triangles x 9
    float *out_spheres;               // n_spheres x 4
};

// rtx::moved_prims on the device, word for word: one launch, one work-item per vertex and one per sphere.  No work-item
// reads what another wrote; every output word has one writer.  On `stream`; nothing is waited for.
hipError_t launch_move(const MoveArgs &a, hipStream_t stream);

}  // namespace rtxf
