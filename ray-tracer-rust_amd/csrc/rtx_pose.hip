// rtx_pose.hip — the posed records of an uploaded scene, made on the device, for gfx950.
//
//   rtx_scene_pose / rtx_scene_pose_device    the primitive records, the shading records and the refitted node stream
//
// The tree keeps its shape, so nothing is sorted or built here: pose_records_kernel restates every triangle from its posed
// vertices (scene_prep.h: triangle_statement, the text the host compiles too), and the refit kernels fold, for every node,
// the own boxes of its contiguous run of records and move the planes outwards by the scene's cull_delta.
//
// The refit folds every range DIRECTLY from the posed primitive records: a node's box depends on no other node's, so the
// only hand-off is the kernel boundary behind pose_records_kernel.  No arrival counters, no spinning, no atomics; every
// output word is written by exactly one work-item.  A range of at most kPoseLaneMax records is folded by one work-item
// (refit_short_kernel); a longer one by one workgroup of kPoseBlock work-items that stride over it and meet in LDS
// (refit_long_kernel), so the root of a 1M-triangle mesh is 4096 steps of a workgroup, not a million of one lane.
//
// The kernels live in namespace rtxp: librtx.so's other kernel sets stay what they were.
#include "rtx_pose.h"

#include <cmath>

namespace rtxp {

using rtx::kPoseBlock;
using rtx::kPoseLaneMax;

__global__ void __launch_bounds__(kPoseBlock) pose_records_kernel(PoseArgs a)
{
    const uint32_t j = blockIdx.x * kPoseBlock + threadIdx.x;
    if (j >= a.n_prims) return;
    rtx::TriRec r = a.tris[j];
    rtx::ShadeRec sh = a.shade[r.idx];
    if (sh.kind == 0u) {
        const float *p = a.pose + 9u * static_cast<size_t>(a.tri_of[r.idx]);
        float v[9];
        for (int k = 0; k < 9; ++k) v[k] = p[k];
        r.v0[0] = v[0];
        r.v0[1] = v[1];
        r.v0[2] = v[2];
        rtx::triangle_statement(v, v + 3, v + 6, r.e1, r.e2, sh.normal, r.bmin, r.bmax);
    }
    sh.rank = a.rank ? a.rank[r.idx] : r.idx;
    a.out_tris[j] = r;
    a.out_shade[r.idx] = sh;
}

// the record of node i: the folded box moved outwards in f32 as rtx::nodes_in_device_order moves it, link and info kept
__device__ inline void write_node(const PoseArgs &a, uint32_t i, const float lo[3], const float hi[3])
{
    const rtx::NodeDev was = a.nodes[i];
    const float d = a.cull_delta;
    a.out_nodes[i] = rtx::NodeDev{lo[0] - d, lo[1] - d, hi[0] + d, hi[1] + d, lo[2] - d, hi[2] + d, was.link, was.info};
}

__global__ void __launch_bounds__(kPoseBlock) refit_short_kernel(PoseArgs a)
{
    const uint32_t k = blockIdx.x * kPoseBlock + threadIdx.x;
    if (k >= a.n_nodes - a.n_long) return;
    const uint32_t i = a.order[a.n_long + k];
    const uint2 range = a.ranges[i];
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (uint32_t j = range.x; j < range.x + range.y; ++j) {
        const rtx::TriRec &t = a.out_tris[j];
        for (int c = 0; c < 3; ++c) {
            lo[c] = fminf(lo[c], t.bmin[c]);
            hi[c] = fmaxf(hi[c], t.bmax[c]);
        }
    }
    write_node(a, i, lo, hi);
}

__global__ void __launch_bounds__(kPoseBlock) refit_long_kernel(PoseArgs a)
{
    __shared__ float part[6][kPoseBlock];
    const uint32_t i = a.order[blockIdx.x];            // blockIdx.x < n_long
    const uint2 range = a.ranges[i];
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (uint32_t j = threadIdx.x; j < range.y; j += kPoseBlock) {
        const rtx::TriRec &t = a.out_tris[range.x + j];
        for (int c = 0; c < 3; ++c) {
            lo[c] = fminf(lo[c], t.bmin[c]);
            hi[c] = fmaxf(hi[c], t.bmax[c]);
        }
    }
    for (int c = 0; c < 3; ++c) {
        part[c][threadIdx.x] = lo[c];
        part[3 + c][threadIdx.x] = hi[c];
    }
    __syncthreads();
    for (uint32_t half = kPoseBlock / 2u; half != 0u; half /= 2u) {
        if (threadIdx.x < half)
            for (int c = 0; c < 3; ++c) {
                part[c][threadIdx.x] = fminf(part[c][threadIdx.x], part[c][threadIdx.x + half]);
                part[3 + c][threadIdx.x] = fmaxf(part[3 + c][threadIdx.x], part[3 + c][threadIdx.x + half]);
            }
        __syncthreads();
    }
    if (threadIdx.x != 0u) return;
    for (int c = 0; c < 3; ++c) {
        lo[c] = part[c][0];
        hi[c] = part[3 + c][0];
    }
    write_node(a, i, lo, hi);
}

hipError_t launch_refit(const PoseArgs &a, hipStream_t stream)
{
    if (a.n_prims == 0u || a.n_nodes == 0u) return hipSuccess;
    if (!a.nodes || !a.ranges || !a.order || !a.out_tris || !a.out_nodes || a.n_long > a.n_nodes) return hipErrorInvalidValue;
    if (a.n_long != 0u) hipLaunchKernelGGL(refit_long_kernel, dim3(a.n_long), dim3(kPoseBlock), 0, stream, a);
    const uint32_t n_short = a.n_nodes - a.n_long;
    if (n_short != 0u)
        hipLaunchKernelGGL(refit_short_kernel, dim3((n_short + kPoseBlock - 1u) / kPoseBlock), dim3(kPoseBlock), 0, stream, a);
    return hipGetLastError();
}

hipError_t launch_pose(const PoseArgs &a, hipStream_t stream)
{
    if (a.n_prims == 0u || a.n_nodes == 0u) return hipSuccess;
    if (!a.tris || !a.shade || !a.nodes || !a.tri_of || !a.ranges || !a.order || !a.pose || !a.out_tris || !a.out_shade ||
        !a.out_nodes || a.n_long > a.n_nodes)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(pose_records_kernel, dim3((a.n_prims + kPoseBlock - 1u) / kPoseBlock), dim3(kPoseBlock), 0, stream, a);
    return launch_refit(a, stream);
}

}  // namespace rtxp
