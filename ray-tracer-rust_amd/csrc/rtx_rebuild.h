// rtx_rebuild.h — the launcher of the rebuild kernels (rtx_rebuild.hip), shared with rtx_api.cpp.
//
// rtx_scene_pose_rebuilt and rtx_scene_pose_rebuilt_device (include/rtx.h) move the triangles of an uploaded scene as
// rtx_scene_pose does and lay a new tree over them: the records of the tree proper are sorted by a 64-bit key of their posed
// own boxes (scene_prep.h: rebuild_key_statement), the shape over the sorted runs is a closed form of the scene's counts
// (rtx::RebuildTables, made once on the host), and the boxes are the refit kernels' fold (rtx_pose.h: launch_refit).  The
// statement both sides compile is scene_prep.h's (rebuild_key_statement, triangle_statement, rebuilt_records).  The kernels
// live in a namespace of their own, rtxb, beside rtx, rtxq, rtxs, rtxv, rtxa, rtxl, rtxt, rtxp and rtxg, whose kernel sets
// stay what they were; the 64-bit sort is instantiated in rtx_rebuild.hip, beside the regrouping pass's 32-bit one in rtx_query.hip.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "scene_prep.h"

namespace rtxb {

constexpr uint32_t kRebuildBlock = 256u;

// the uploaded scene (read only), the pose's table (rtx::PoseTables::tri_of, on the device), the call's arrays, the sort's
// buffers and the pose's records (library-owned, written by the kernels)
struct RebuildArgs {
    const rtx::TriRec *tris;          // n_prims uploaded records, leaf order
    const rtx::ShadeRec *shade;       // n_prims, Vec order
    const uint32_t *tri_of;           // n_prims
    uint32_t n_prims, n_global;       // the tree proper: records [n_global, n_prims)
    float bound, scale;               // rebuild_key_statement's M and S
    const float *pose;                // n_tris x 9, the caller's
    const uint32_t *rank;             // n_prims per Vec position, or NULL: the position
    uint64_t *keys, *keys_sorted;     // n_prims - n_global each
    uint32_t *index;                  // n_prims - n_global: the source positions, n_global ...
    uint32_t *perm;                   // n_prims - n_global: the same by rising key (rtx_debug_pose_rebuilt reads it)
    void *temp;                       // the sort's temporary storage (sort_temp_bytes)
    size_t temp_bytes;
    rtx::TriRec *out_tris;            // n_prims, sorted order
    rtx::ShadeRec *out_shade;         // n_prims, Vec order
};

// temporary storage the sort wants for n (key, source position) pairs
hipError_t sort_temp_bytes(uint32_t n_entries, size_t *bytes);

// rtx::rebuilt_records' keys, permutation and records on the device, word for word: key_kernel (one work-item per record
// of the tree proper), the radix sort of (key, source position), records_kernel (one work-item per record: position j of
// the sorted array is made from source position perm[j - n_global], a global triangle from its own).  A kernel boundary is
// the only hand-off: no work-item reads what another workgroup wrote in the same launch.  The boxes are not made here:
// rtxp::launch_refit follows over out_tris.  All on `stream`; nothing is waited for.
hipError_t launch_rebuild(const RebuildArgs &a, hipStream_t stream);

}  // namespace rtxb
