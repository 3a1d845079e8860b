// rtx_prims.hip — the overlay of a pose that states every field of a primitive, made on the device, for gfx950.
//
//   rtx_scene_pose_prims / rtx_scene_pose_prims_device    the uploaded records with spheres restated and colours replaced
//
// overlay_kernel makes, for every record of the uploaded primitive array, the record the pose and rebuild kernels are to
// take for the uploaded one: a sphere restated from the call's {origin, radius} (scene_prep.h: sphere_statement, the text
// the host compiles too), an rgb replaced from the call's colour array of the record's arm, every other word copied.  The
// pose kernels (rtx_pose.hip) or the rebuild kernels (rtx_rebuild.hip) follow behind it on the same stream and read the
// overlay through their `tris` / `shade` pointers; the kernel boundary is the only hand-off.
//
// One record per work-item, memory-bound: 64 + 32 bytes read and as many written, plus the call's arrays.  A primitive
// record is read and written as four 16-byte words, a shading record as two (the records lie on 64- and 32-byte
// boundaries of the library's allocations).  No arrival counters, no spinning, no atomics; every output word is written
// by exactly one work-item, and no work-item reads what another wrote.
//
// The kernel lives in namespace rtxm: librtx.so's other kernel sets stay what they were.
#include "rtx_prims.h"

namespace rtxm {

union RecordWords {
    rtx::TriRec rec;
    uint4 w[4];
    __device__ RecordWords() : w{} {}
};
static_assert(sizeof(RecordWords) == 64, "a primitive record is four 16-byte words");
union ShadeWords {
    rtx::ShadeRec rec;
    uint4 w[2];
    __device__ ShadeWords() : w{} {}
};
static_assert(sizeof(ShadeWords) == 32, "a shading record is two 16-byte words");

__global__ void __launch_bounds__(kOverlayBlock) overlay_kernel(OverlayArgs a)
{
    const uint32_t j = blockIdx.x * kOverlayBlock + threadIdx.x;
    if (j >= a.n_prims) return;
    const bool records = a.spheres != nullptr;          // (uniform: without posed spheres only the shading half is made)
    RecordWords r;
    if (records) {
        const uint4 *p = reinterpret_cast<const uint4 *>(a.tris + j);
        for (int k = 0; k < 4; ++k) r.w[k] = p[k];
    } else {
        r.rec.idx = a.tris[j].idx;
    }
    const uint32_t idx = r.rec.idx;
    ShadeWords sh;
    {
        const uint4 *p = reinterpret_cast<const uint4 *>(a.shade + idx);
        sh.w[0] = p[0];
        sh.w[1] = p[1];
    }
    const float *colour = nullptr;
    if (sh.rec.kind != 0u) {
        if (a.spheres || a.sphere_rgb) {
            const size_t n = a.sphere_of[idx];
            if (a.spheres) {
                const float *s = a.spheres + 4u * n;
                const float in[4] = {s[0], s[1], s[2], s[3]};
                rtx::sphere_statement(in, r.rec.v0, r.rec.e1, r.rec.bmin, r.rec.bmax, sh.rec.normal);
            }
            if (a.sphere_rgb) colour = a.sphere_rgb + 3u * n;
        }
    } else if (a.rgb) {
        colour = a.rgb + 3u * static_cast<size_t>(a.tri_of[idx]);
    }
    if (colour)
        for (int k = 0; k < 3; ++k) sh.rec.rgb[k] = colour[k];
    if (records) {
        uint4 *out = reinterpret_cast<uint4 *>(a.ov_tris + j);
        for (int k = 0; k < 4; ++k) out[k] = r.w[k];
    }
    uint4 *out = reinterpret_cast<uint4 *>(a.ov_shade + idx);
    out[0] = sh.w[0];
    out[1] = sh.w[1];
}

hipError_t launch_overlay(const OverlayArgs &a, hipStream_t stream)
{
    if (a.n_prims == 0u || (!a.spheres && !a.rgb && !a.sphere_rgb)) return hipSuccess;
    if (!a.tris || !a.shade || !a.ov_shade || (a.rgb && !a.tri_of) || ((a.spheres || a.sphere_rgb) && !a.sphere_of) ||
        (a.spheres && !a.ov_tris))
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(overlay_kernel, dim3((a.n_prims + kOverlayBlock - 1u) / kOverlayBlock), dim3(kOverlayBlock), 0, stream, a);
    return hipGetLastError();
}

}  // namespace rtxm
