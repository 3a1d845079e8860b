// rtx_view.h — the launcher of the view kernels (rtx_view.hip), shared with rtx_api.cpp.
//
// rtx_render_view (include/rtx.h) renders a rectangle of ANY pinhole view of an uploaded scene: create_rays' rays
// (main.rs:151-178) for the view's frame and camera, made in registers, through render_pixel's body
// (rtx_shade_pixel.hpp).  Its kernels live in a namespace of their own, rtxv, beside the render pipeline's (rtx), the ray
// queries' (rtxq) and ray shading's (rtxs), whose kernel sets stay what they were.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "rtx_device.h"

namespace rtxv {

// RtxView (include/rtx.h), field for field: passed to the kernel by value
struct ViewBlock {
    uint32_t width, height;
    float eye[3], u[3], v[3], w[3];
    float distance;
    uint32_t x0, y0, nx, ny;
};
static_assert(sizeof(ViewBlock) == 76, "ViewBlock is RtxView");

constexpr uint32_t kMaxRays = 1u << 28;      // rays of one launch (rtxq::kMaxRays): record numbers stay below 2^32 bytes / 16

// Pixels [x0, x0+nx) x [y0, y0+ny) of the view, nx * ny * S.nb_ray <= kMaxRays, nx, ny > 0; pixel (x, y) is record
// (y-y0)*nx + (x-x0) of the outputs.  d_rgb: NULL or nx*ny*3 bytes; d_shade: NULL or nx*ny RtxPixelShade (16-byte aligned);
// d_hits: NULL or nx*ny*nb_ray RtxRayHit (16-byte aligned), a pixel's rays consecutive; counters: NULL or
// rtx::kNumCounters words the kernel ADDS to, as rtxs::launch_shade; origin_bound: as rtxq::launch_query — the eye is
// compared with it here, once for the launch.
hipError_t launch_view(const rtx::DeviceScene &S, const ViewBlock &V, float origin_bound, void *d_rgb, void *d_shade,
                       void *d_hits, unsigned long long *counters, hipStream_t stream);

}  // namespace rtxv
