// rtx_shade.h — the launcher of the ray-shading kernels (rtx_shade.hip), shared with rtx_api.cpp.
//
// rtx_shade_rays (include/rtx.h) runs render_pixel's body (main.rs:186-236) for rays the CALLER supplies: closest hit,
// nb_light_sample shadow rays towards the area light, the ordered f32 sum, the gamma table.  Its kernels live in a
// namespace of their own, rtxs, beside the render pipeline's (rtx) and the ray queries' (rtxq), whose kernel sets stay
// what they were.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "rtx_device.h"
#include "rtx_query.h"

namespace rtxs {

// One batch of n_pixels pixels, S.nb_ray consecutive rays each (n_pixels * S.nb_ray <= rtxq::kMaxRays).  origins,
// directions: n_pixels * nb_ray x 3 floats; out_shade: n_pixels RtxPixelShade (16-byte aligned); out_hits: NULL or
// n_pixels * nb_ray RtxRayHit (16-byte aligned), the records rtx_trace_rays writes for the same rays; sort: NULL = shade
// in the caller's order, else the regrouping pass's buffers (rtx_query.h), sized for n_pixels at least — the key is built
// from each pixel's ray 0; counters: NULL or rtx::kNumCounters words the kernel ADDS to ([0] primary hits, [1..4] as the
// render kernels, [5] 64-lane walks, primary or shadow, that took the reference traversal); box, origin_bound: as
// rtxq::launch_query.
hipError_t launch_shade(const rtx::DeviceScene &S, uint32_t n_pixels, const float *origins, const float *directions,
                        const rtxq::KeyBox &box, float origin_bound, const rtxq::SortBuffers *sort, void *out_shade,
                        void *out_hits, unsigned long long *counters, hipStream_t stream);

}  // namespace rtxs
