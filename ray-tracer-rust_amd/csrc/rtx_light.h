// rtx_light.h — the launcher of the light kernel (rtx_light.hip), shared with rtx_api.cpp.
//
// rtx_render_view_lit and rtx_shade_rays_lit (include/rtx.h) shade with a light other than the one rtx_scene_create was
// given.  rtxv::view_kernel and rtxs::shade_kernel read the light as its points and their count alone
// (rtx_shade_pixel.hpp: S.light_points, S.nb_light), so a lit call is the same kernels with those two fields of their
// DeviceScene copy swapped; what it needs made is the points, on the device, on the call's stream.  The kernel lives in a
// namespace of its own, rtxl, beside rtx, rtxq, rtxs, rtxv and rtxa, whose kernel sets stay what they were.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "scene_prep.h"

namespace rtxl {

// Light.primitives[0]: v0, v1, v2 — the first 36 bytes of an RtxLight, handed to the kernel as an argument
struct LightTriangle {
    float v[9];
};
static_assert(sizeof(LightTriangle) == 36, "the triangle of an RtxLight");

// out[3 * (r * nb_light + i)] = rtx::light_sample_point(tri, samples[(r * nb_ray + i) % n_samples]) for r < nb_ray,
// i < nb_light: rtx::light_points_of (scene_prep.cpp) on the device, bit for bit — both compile scene_prep.h's one
// statement.  samples: the uploaded table, n_samples pairs; out: nb_ray * nb_light x 3 floats.  One launch on `stream`;
// nb_ray * nb_light == 0: nothing.  More than rtx::kMaxCallLightPoints points, or n_samples == 0: hipErrorInvalidValue.
hipError_t launch_light_points(const float2 *samples, uint32_t n_samples, const LightTriangle &tri, uint32_t nb_ray,
                               uint32_t nb_light, float *out, hipStream_t stream);

}  // namespace rtxl
