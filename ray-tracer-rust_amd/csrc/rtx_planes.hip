// rtx_planes.hip — the plane records of a pose's global triangles, made on the device, for gfx950.
//
//   rtx_scene_pose / rtx_scene_pose_device    ... behind the pose kernels: what rtx_render_view_rows_posed's shading pass
//                                             reads of the first global triangle (rtx_traverse.hpp: plane_rules_out)
//
// At most rtx::kMaxGlobalPrims records: one work-item each, one workgroup.  All arithmetic is scene_prep.h's
// global_plane_statement, in double: v_cvt_f64_f32 of the edges, products that are exact, one rounding per sum, v_cvt_f32_f64
// to nearest, and the step upwards as an increment of the bit pattern.  The unit is compiled like every other one — no
// contraction, no flushing: a ground at constant height has W components that are exactly 0, whose successor is the smallest
// f32 subnormal and enters the sum behind K_d as it is (the kernel's denormal mode keeps f32 and f64 subnormals).
//
// The kernel lives in namespace rtxg: librtx.so's other kernel sets stay what they were.
#include "rtx_planes.h"

namespace rtxg {

constexpr uint32_t kPlanesBlock = 64u;

__global__ void __launch_bounds__(kPlanesBlock) global_planes_kernel(const rtx::TriRec *tris, uint32_t n_global, rtx::TriRec *out)
{
    const uint32_t i = blockIdx.x * kPlanesBlock + threadIdx.x;
    if (i >= n_global) return;
    rtx::global_plane_statement(tris[i], out + i);
}

hipError_t launch_global_planes(const rtx::TriRec *tris, uint32_t n_global, rtx::TriRec *out, hipStream_t stream)
{
    if (n_global == 0u) return hipSuccess;
    if (!tris || !out) return hipErrorInvalidValue;
    hipLaunchKernelGGL(global_planes_kernel, dim3((n_global + kPlanesBlock - 1u) / kPlanesBlock), dim3(kPlanesBlock), 0, stream,
                       tris, n_global, out);
    return hipGetLastError();
}

}  // namespace rtxg
