// rtx_skin.hip — a pose's vertices and spheres made on the device from the rest geometry, the scene's skin and a set of
// moves, for gfx950.
//
//   rtx_scene_pose_skinned / rtx_scene_pose_skinned_device    the arrays rtx_scene_pose_prims_device is then handed
//
// skin_kernel runs scene_prep.h's skin_statement — the text the host compiles too — over every corner of the scene's
// triangles as created, and move_statement over every sphere under the skin's sphere_bone.  It writes the two buffers
// rtxf::move_kernel writes, and the overlay kernel (rtx_prims.hip) and the pose or rebuild kernels (rtx_pose.hip,
// rtx_rebuild.hip) follow behind it on the same stream; the kernel boundary is the only hand-off.
//
// One work-item per CORNER, then one per sphere.  A corner reads its rest vertex (12 bytes), its four bones and its four
// weights (one 16-byte load each: the skin's buffers are the library's, 16-byte aligned, 32 bytes per corner in corner
// order) and writes 12 bytes: a wavefront reads 768 + 1,024 + 1,024 and writes 768 contiguous bytes.  The bones are per
// corner and so not wave-uniform: the 48 bytes of a move are vector loads behind the compare against n_moves, which the
// cache serves — a skeleton's moves are a few lines.  A bone out of range reads no move (move_statement).  No arrival
// counters, no spinning, no atomics, no LDS; every output word is written by exactly one work-item, and no work-item reads
// what another wrote.
//
// The kernel lives in namespace rtxk: librtx.so's other kernel sets stay what they were.
#include "rtx_skin.h"

namespace rtxk {

__global__ void __launch_bounds__(kSkinBlock) skin_kernel(SkinArgs a)
{
    const uint32_t i = blockIdx.x * kSkinBlock + threadIdx.x;
    const uint32_t n_corners = 3u * a.n_triangles;
    if (i < n_corners) {
        const uint4 b = a.bones[i];
        const float4 w = a.weights[i];
        const uint32_t bones[4] = {b.x, b.y, b.z, b.w};
        const float weights[4] = {w.x, w.y, w.z, w.w};
        const float *p = a.rest_v + 3u * static_cast<size_t>(i);
        const float in[3] = {p[0], p[1], p[2]};
        float out[3];
        rtx::skin_statement(a.moves, a.n_moves, bones, weights, in, out);
        float *q = a.out_v + 3u * static_cast<size_t>(i);
        for (int k = 0; k < 3; ++k) q[k] = out[k];
        return;
    }
    const uint32_t s = i - n_corners;
    if (s >= a.n_spheres) return;
    const float *p = a.rest_spheres + 4u * static_cast<size_t>(s);
    const float in[4] = {p[0], p[1], p[2], p[3]};
    float out[4];
    rtx::move_statement(a.moves, a.radius_scale, a.n_moves, a.sphere_bone[s], true, in, out);
    float *q = a.out_spheres + 4u * static_cast<size_t>(s);
    for (int k = 0; k < 4; ++k) q[k] = out[k];
}

hipError_t launch_skin(const SkinArgs &a, hipStream_t stream)
{
    const uint64_t n = 3ull * a.n_triangles + a.n_spheres;
    if (n == 0u) return hipSuccess;
    if (!a.moves || a.n_moves == 0u || a.n_moves > rtx::kMaxMoves ||
        (a.n_triangles && (!a.rest_v || !a.out_v || !a.bones || !a.weights)) ||
        (a.n_spheres && (!a.rest_spheres || !a.out_spheres || !a.sphere_bone)) ||
        ((reinterpret_cast<uintptr_t>(a.bones) | reinterpret_cast<uintptr_t>(a.weights)) & 15u) || n > 0xFFFFFFFFull - kSkinBlock)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(skin_kernel, dim3(static_cast<uint32_t>((n + kSkinBlock - 1u) / kSkinBlock)), dim3(kSkinBlock), 0, stream, a);
    return hipGetLastError();
}

}  // namespace rtxk
