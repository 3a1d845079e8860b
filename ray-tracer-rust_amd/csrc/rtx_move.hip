// rtx_move.hip — a pose's vertices and spheres made on the device from the rest geometry and a set of moves, for gfx950.
//
//   rtx_scene_pose_moved / rtx_scene_pose_moved_device    the arrays rtx_scene_pose_prims_device is then handed
//
// move_kernel runs scene_prep.h's move_statement — the text the host compiles too — over every vertex of the scene's
// triangles as created and over every sphere.  The overlay kernel (rtx_prims.hip) and the pose or rebuild kernels
// (rtx_pose.hip, rtx_rebuild.hip) follow behind it on the same stream and read its two arrays where they read a
// caller's; the kernel boundary is the only hand-off.
//
// One work-item per VERTEX, then one per sphere: 12 bytes in and 12 out, neighbouring work-items on neighbouring
// addresses, so a wavefront reads and writes 768 contiguous bytes.  The three work-items of a triangle read the same
// tri_vec and group words (one request each, served as a broadcast).  The move index is per primitive and so not
// wave-uniform: the 48 bytes of a move are a vector load, which the cache serves — a handful of moves is a few lines.
// The index is compared against n_moves before it is used (move_statement): a value out of range copies the words.
// No arrival counters, no spinning, no atomics, no LDS; every output word is written by exactly one work-item, and no
// work-item reads what another wrote.
//
// The kernel lives in namespace rtxf: librtx.so's other kernel sets stay what they were.
#include "rtx_move.h"

namespace rtxf {

__global__ void __launch_bounds__(kMoveBlock) move_kernel(MoveArgs a)
{
    const uint32_t i = blockIdx.x * kMoveBlock + threadIdx.x;
    const uint32_t n_vertices = 3u * a.n_triangles;
    if (i < n_vertices) {
        const uint32_t g = a.group ? a.group[a.tri_vec[i / 3u]] : 0u;
        const float *p = a.rest_v + 3u * static_cast<size_t>(i);
        const float in[3] = {p[0], p[1], p[2]};
        float out[3];
        rtx::move_statement(a.moves, a.radius_scale, a.n_moves, g, false, in, out);
        float *q = a.out_v + 3u * static_cast<size_t>(i);
        for (int k = 0; k < 3; ++k) q[k] = out[k];
        return;
    }
    const uint32_t s = i - n_vertices;
    if (s >= a.n_spheres) return;
    const uint32_t g = a.group ? a.group[a.sphere_vec[s]] : 0u;
    const float *p = a.rest_spheres + 4u * static_cast<size_t>(s);
    const float in[4] = {p[0], p[1], p[2], p[3]};
    float out[4];
    rtx::move_statement(a.moves, a.radius_scale, a.n_moves, g, true, in, out);
    float *q = a.out_spheres + 4u * static_cast<size_t>(s);
    for (int k = 0; k < 4; ++k) q[k] = out[k];
}

hipError_t launch_move(const MoveArgs &a, hipStream_t stream)
{
    const uint64_t n = 3ull * a.n_triangles + a.n_spheres;
    if (n == 0u) return hipSuccess;
    if (!a.moves || a.n_moves == 0u || a.n_moves > rtx::kMaxMoves || (a.n_triangles && (!a.rest_v || !a.out_v)) ||
        (a.n_spheres && (!a.rest_spheres || !a.out_spheres)) ||
        (a.group && ((a.n_triangles && !a.tri_vec) || (a.n_spheres && !a.sphere_vec))) || n > 0xFFFFFFFFull - kMoveBlock)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(move_kernel, dim3(static_cast<uint32_t>((n + kMoveBlock - 1u) / kMoveBlock)), dim3(kMoveBlock), 0, stream, a);
    return hipGetLastError();
}

}  // namespace rtxf
