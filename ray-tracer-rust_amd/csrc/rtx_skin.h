// rtx_skin.h — the launcher of the skin kernel (rtx_skin.hip), shared with rtx_api.cpp.
//
// rtx_scene_pose_skinned and rtx_scene_pose_skinned_device (include/rtx.h) make a pose's vertices and spheres on the
// device as a moved pose does (rtx_move.h), with one difference: every triangle CORNER blends up to four moves by the
// weights of the scene's skin (rtx_scene_skin, uploaded once per bind and device), and every sphere follows the skin's
// sphere_bone.  The kernel writes the two arrays the move kernel writes, and everything behind it runs as for any pose.
// The statement both sides compile is scene_prep.h's skin_statement.  The kernel lives in a namespace of its own, rtxk,
// beside rtx, rtxq, rtxs, rtxv, rtxa, rtxl, rtxt, rtxp, rtxg, rtxb, rtxm and rtxf, whose kernel sets stay what they were.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "scene_prep.h"

namespace rtxk {

constexpr uint32_t kSkinBlock = 256u;

// the rest geometry and the skin (read only, library-owned, the skin's arrays 16-byte aligned), the call's arrays and the
// two output buffers (library-owned, written by the kernel)
struct SkinArgs {
    const float *rest_v;              // n_triangles x 9
    const float *rest_spheres;        // n_spheres x 4
    const uint4 *bones;               // n_triangles x 3: a corner's four bones
    const float4 *weights;            // n_triangles x 3: a corner's four weights
    const uint32_t *sphere_bone;      // n_spheres
    uint32_t n_triangles, n_spheres;
    uint32_t n_moves;
    const float *moves;               // n_moves x 12
    const float *radius_scale;        // NULL or n_moves
    float *out_v;                     // n_triangles x 9
    float *out_spheres;               // n_spheres x 4
};

// rtx::skinned_prims on the device, word for word: one launch, one work-item per corner and one per sphere.  No work-item
// reads what another wrote; every output word has one writer.  On `stream`; nothing is waited for.
hipError_t launch_skin(const SkinArgs &a, hipStream_t stream);

}  // namespace rtxk
