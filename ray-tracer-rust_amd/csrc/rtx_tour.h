// rtx_tour.h — the launchers of the walk kernels (rtx_tour.hip), shared with rtx_api.cpp.
//
// rtx_render_view_rows_lit (include/rtx.h) renders through the render pipeline with a light other than the one
// rtx_scene_create was given.  The pipeline's kernels (rtx_kernel.hip) read the light as five fields of their DeviceScene
// copy — light_points, light_tour, light_boxes, shaft_delta, nb_light — so a lit pipeline call is the same kernels with
// those swapped.  The points are rtxl::light_points_kernel's; the margin is a scalar the host computes; the tour and the
// boxes are made here, on the device, on the call's stream.  The kernels live in a namespace of their own, rtxt, beside
// rtx, rtxq, rtxs, rtxv, rtxa and rtxl, whose kernel sets stay what they were.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "scene_prep.h"

namespace rtxt {

// tour[4 * (r * nb_light + b0 + k)] .. + 3 = {points[r * nb_light + b0 + o[k]] xyz, o[k] as bits} for every primary ray
// r < nb_ray and every batch [b0, b0 + n) of n = min(nb_light - b0, rtx::kMaxLightBatch) consecutive samples, o =
// rtx::light_tour_order_f32 of the batch's points: the host's scan word for word (both compile scene_prep.h's
// tour_distance).  points: nb_ray * nb_light x 3 floats; tour: as many 16-byte records, 16-byte aligned.  One launch on
// `stream`, one workgroup of one wavefront per batch; nb_ray * nb_light == 0: nothing.  More than
// rtx::kMaxCallLightPoints points: hipErrorInvalidValue.
hipError_t launch_tour(const float *points, uint32_t nb_ray, uint32_t nb_light, float *tour, hipStream_t stream);

// boxes[6 * r] .. + 5 = lo xyz, hi xyz of the nb_light points of primary ray r: rtx::light_boxes_of by value (fmin / fmax
// from -+infinity, a NaN ignored; the sign of a zero bound is not defined).  One launch on `stream`, one wavefront per ray;
// the same bounds as launch_tour.
hipError_t launch_light_boxes(const float *points, uint32_t nb_ray, uint32_t nb_light, float *boxes, hipStream_t stream);

}  // namespace rtxt
