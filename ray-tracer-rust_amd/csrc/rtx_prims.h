// rtx_prims.h — the launcher of the overlay kernel (rtx_prims.hip), shared with rtx_api.cpp.
//
// rtx_scene_pose_prims and rtx_scene_pose_prims_device (include/rtx.h) pose every field of every primitive: the triangles'
// vertices as rtx_scene_pose does, and beside them the spheres' origins and radii and both arms' colours.  The pose and
// rebuild kernels (rtx_pose.hip, rtx_rebuild.hip) copy what they do not restate — a sphere's record, a record's rgb, a
// sphere's key from its own box — from the arrays they are handed as the uploaded ones, so what such a pose needs made is
// an OVERLAY of those arrays: the uploaded records with the spheres restated (scene_prep.h: sphere_statement, the text
// the host compiles too) and the colours replaced.  The existing kernels then run unchanged over the overlay.  The
// statement both sides compile is scene_prep.h's (sphere_statement, PrimsOverlay, overlay_records).  The kernel lives in
// a namespace of its own, rtxm, beside rtx, rtxq, rtxs, rtxv, rtxa, rtxl, rtxt, rtxp, rtxg and rtxb, whose kernel sets stay
// what they were.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "scene_prep.h"

namespace rtxm {

constexpr uint32_t kOverlayBlock = 256u;

// the uploaded scene (read only), the host tables (rtx::PoseTables, on the device), the call's arrays and the overlay's
// buffers (library-owned, written by the kernel)
struct OverlayArgs {
    const rtx::TriRec *tris;          // n_prims uploaded records, leaf order
    const rtx::ShadeRec *shade;       // n_prims, Vec order
    const uint32_t *tri_of;           // n_prims: Vec position -> triangle number (read when rgb is given)
    const uint32_t *sphere_of;        // n_prims: Vec position -> sphere number (read when spheres or sphere_rgb is given)
    uint32_t n_prims;
    const float *spheres;             // NULL or n_spheres x 4: origin x, y, z, radius
    const float *rgb;                 // NULL or n_triangles x 3
    const float *sphere_rgb;          // NULL or n_spheres x 3
    rtx::TriRec *ov_tris;             // n_prims, leaf order; written (and required) only when spheres is given
    rtx::ShadeRec *ov_shade;          // n_prims, Vec order
};

// rtx::overlay_records on the device, word for word: one launch, one work-item per record of the primitive array.  No
// work-item reads what another wrote; every output word has one writer (a Vec position occurs once in leaf order).  With
// none of the three arrays given nothing is launched.  On `stream`; nothing is waited for.
hipError_t launch_overlay(const OverlayArgs &a, hipStream_t stream);

}  // namespace rtxm
