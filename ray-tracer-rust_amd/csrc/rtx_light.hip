// rtx_light.hip — the light points of any area light, made on the device, for gfx950.
//
//   rtx_render_view_lit    rtxv::view_kernel with another light's points and count
//   rtx_shade_rays_lit     rtxs::shade_kernel with the same
//
// The reference draws a shadow ray's target inside the shadow loop: Light::get_sample(T[(r*NB_RAY + i) % len])
// (main.rs:194-196, light.rs:11-13, triangle.rs:113-127).  The index does not depend on the pixel, so the nb_ray x
// nb_light points are the same for every pixel; rtx_scene_create makes them once on the host (scene_prep.cpp:
// light_points_of).  For a light given per call they are made here instead, from the uploaded sample table and the 36
// bytes of the triangle in the argument block: the device-resident entry points are asynchronous on the caller's stream,
// and a table made on the host would need a pinned staging area with a lifetime of its own.
//
// One work-item makes one point.  No LDS, no atomics, every output float written by exactly one work-item.
//
// The kernel lives in namespace rtxl: librtx.so's rtx::, rtxq::, rtxs::, rtxv:: and rtxa:: kernel sets stay what they were.
#include "rtx_light.h"

namespace rtxl {

constexpr uint32_t kLightBlock = 256u;

// point p = r * nb_light + i, p < n_points = nb_ray * nb_light <= 2^20; the table index in 64 bits, as the host has it
__global__ void __launch_bounds__(kLightBlock) light_points_kernel(const float2 *__restrict__ samples, uint32_t n_samples,
                                                                   LightTriangle tri, uint32_t nb_ray, uint32_t nb_light,
                                                                   uint32_t n_points, float *__restrict__ out)
{
    const uint32_t p = blockIdx.x * kLightBlock + threadIdx.x;
    if (p >= n_points) return;
    const uint32_t r = p / nb_light, i = p - r * nb_light;
    const float2 s = samples[(static_cast<uint64_t>(r) * nb_ray + i) % n_samples];      // main.rs:195
    float q[3];
    rtx::light_sample_point(tri.v, tri.v + 3, tri.v + 6, s.x, s.y, q);
    float *o = out + 3u * static_cast<size_t>(p);
    o[0] = q[0];
    o[1] = q[1];
    o[2] = q[2];
}

hipError_t launch_light_points(const float2 *samples, uint32_t n_samples, const LightTriangle &tri, uint32_t nb_ray,
                               uint32_t nb_light, float *out, hipStream_t stream)
{
    const uint64_t n_points = static_cast<uint64_t>(nb_ray) * nb_light;
    if (n_points == 0u) return hipSuccess;
    if (!samples || !out || n_samples == 0u || n_points > rtx::kMaxCallLightPoints) return hipErrorInvalidValue;
    const uint32_t n = static_cast<uint32_t>(n_points);
    hipLaunchKernelGGL(light_points_kernel, dim3((n + kLightBlock - 1u) / kLightBlock), dim3(kLightBlock), 0, stream, samples,
                       n_samples, tri, nb_ray, nb_light, n, out);
    return hipGetLastError();
}

}  // namespace rtxl
