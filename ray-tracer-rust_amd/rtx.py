"""ctypes binding of librtx.so (include/rtx.h) — the Python face of the C ABI.

Plumbing only: every ray is traced by the HIP kernel inside librtx.so.  There is
no Python or CPU rendering path; if the library is missing, importing this
module fails loudly, and rendering without a GPU raises RtxError(NO_DEVICE).

Names mirror the reference (antoinedesbois/Ray-Tracer-Rust): Scene{width,height,
light,camera,bvh} (src/tracer/utils/scene.rs:6-12) is flattened into
RtxSceneDesc; the default-scene literals are those of main() (src/main.rs:327-358).
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# librtx.so is the product.  RTX_PY_ABLATION=1 makes THIS BINDING load librtx_ablation.so instead (the same sources
# built with -DRTX_ABLATION=1: every earlier kernel form, selectable through RTX_VARIANT) — for tools/ and the
# variant-equality test only; the library itself reads no environment variable.  RTX_PY_LIB=<path> makes this binding
# load a library built somewhere else (tools/ab_build.sh: A/B variants live under gpurun_out/ and never replace the
# product's file).
LIB_PATH = os.environ.get("RTX_PY_LIB") or os.path.join(
    _HERE, "librtx_ablation.so" if os.environ.get("RTX_PY_ABLATION") == "1" else "librtx.so")

if not os.path.exists(LIB_PATH):
    raise ImportError(
        "%s is not built. Build it with: python -c 'import __graft_entry__ as g; g.build()' "
        "or make -C ray-tracer-rust_amd/csrc [ablation]" % LIB_PATH)

_lib = C.CDLL(LIB_PATH)

OK, ERR_BAD_ARG, ERR_NO_DEVICE, ERR_HIP, ERR_OOM, ERR_UNSUPPORTED, ERR_INTERNAL, ERR_IO = 0, -1, -2, -3, -4, -5, -6, -7
ACCEL_BVH, ACCEL_BRUTE = 0, 1
REFTREE_AUTO, REFTREE_ALWAYS, REFTREE_NEVER = 0, 1, 2

# constants of the reference: src/main.rs:38-40
NB_RAY, NB_LIGHT_SAMPLE, NB_RAND_SAMPLE = 1, 100, 2000000
# default scene: camera src/main.rs:353-356, light :337-343, ground :102-111, frame :350-351
DEFAULT_EYE = (0.0, 100.0, 200.0)
DEFAULT_LOOK_AT = (0.0, 0.0, -100000.0)
DEFAULT_UP = (0.0, 1.0, 0.0)
DEFAULT_DISTANCE = 288.0
DEFAULT_LIGHT = (-10.0, 300.0, -10.0, 10.0, 300.0, -10.0, 0.0, 300.0, 0.0)
GROUND_TRI = (-10000.0, 0.0, -10000.0, 10000.0, 0.0, -10000.0, 0.0, 0.0, 10000.0)
GROUND_RGB = (0.5, 0.5, 0.5)
MESH_RGB = (1.0, 1.0, 1.0)
DEFAULT_WIDTH, DEFAULT_HEIGHT = 1920, 1080
DEFAULT_SEED = 20261004

f32p = C.POINTER(C.c_float)
u32p = C.POINTER(C.c_uint32)
u8p = C.POINTER(C.c_uint8)
u64p = C.POINTER(C.c_uint64)


class SceneDesc(C.Structure):
    _fields_ = [
        ("width", C.c_uint32), ("height", C.c_uint32),
        ("eye", C.c_float * 3), ("u", C.c_float * 3), ("v", C.c_float * 3), ("w", C.c_float * 3),
        ("distance", C.c_float),
        ("light_v0", C.c_float * 3), ("light_v1", C.c_float * 3), ("light_v2", C.c_float * 3),
        ("n_tris", C.c_uint32),
        ("v0v1v2", f32p), ("rgb", f32p), ("tie_rank", u32p),
        ("nb_ray", C.c_uint32), ("nb_light_sample", C.c_uint32),
        ("samples", f32p), ("n_samples", C.c_uint32),
        ("accel", C.c_uint32), ("leaf_max", C.c_uint32), ("reference_tree", C.c_uint32),
        ("n_spheres", C.c_uint32), ("spheres", f32p), ("sphere_rgb", f32p), ("kinds", u8p),
    ]


class Stats(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in (
        "primary_rays", "primary_hits", "shadow_rays", "rays", "box_tests", "tri_tests",
        "wave_node_visits", "wave_tri_visits", "redo_tiles")] + [("kernel_ms", C.c_double), ("total_ms", C.c_double)]

    def asdict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


class SceneInfo(C.Structure):
    _fields_ = [(n, C.c_uint32) for n in ("n_tris", "n_nodes", "n_leaves", "max_leaf_tris", "depth", "n_light_points",
                                          "n_ref_nodes", "n_global")] + \
               [(n, C.c_uint64) for n in ("node_bytes", "tri_bytes", "shade_bytes", "sample_bytes")]

    def asdict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


class RayHit(C.Structure):
    """RtxRayHit: one closest hit (prim == NO_HIT: a miss, everything else zero)."""
    _fields_ = [("prim", C.c_uint32), ("t", C.c_float), ("p_hit", C.c_float * 3), ("normal", C.c_float * 3)]


NO_HIT = 0xFFFFFFFF
RAYS_KEEP_ORDER, RAYS_FORCE_REGROUP = 1, 2
# the refit kernels' size thresholds (scene_prep.h: kPoseLaneMax, kPoseBlock): a node whose run of records is longer than
# POSE_LANE_MAX is folded by one workgroup of POSE_BLOCK work-items, a shorter one by one work-item
POSE_LANE_MAX, POSE_BLOCK = 32, 256
# the same 32 bytes as a numpy record: what Scene.trace_rays returns
RAY_HIT_DTYPE = np.dtype([("prim", np.uint32), ("t", np.float32), ("p_hit", np.float32, 3), ("normal", np.float32, 3)])
assert RAY_HIT_DTYPE.itemsize == C.sizeof(RayHit) == 32


class PixelShade(C.Structure):
    """RtxPixelShade: render_pixel's result for one pixel of caller-supplied rays."""
    _fields_ = [("linear", C.c_float * 3), ("rgb8", C.c_uint8 * 3), ("hits", C.c_uint8)]


# the same 16 bytes as a numpy record: what Scene.shade_rays returns
PIXEL_SHADE_DTYPE = np.dtype([("linear", np.float32, 3), ("rgb8", np.uint8, 3), ("hits", np.uint8)])
assert PIXEL_SHADE_DTYPE.itemsize == C.sizeof(PixelShade) == 16


class AccumPixel(C.Structure):
    """RtxAccumPixel: a pixel's ordered sum over the frames added so far and in how many of them it had a hit."""
    _fields_ = [("sum", C.c_float * 3), ("hit_frames", C.c_uint32)]


# the same 16 bytes as a numpy record: what accum_add works on
ACCUM_PIXEL_DTYPE = np.dtype([("sum", np.float32, 3), ("hit_frames", np.uint32)])
assert ACCUM_PIXEL_DTYPE.itemsize == C.sizeof(AccumPixel) == 16
MAX_MEAN_FRAMES = 65536
MEAN_POSED = 1
ADAPT_CONTINUE = 2


class MomentPixel(C.Structure):
    """RtxMomentPixel: RtxAccumPixel's words, the ordered sum of the frames' squared linear colours and the pixel's own count."""
    _fields_ = [("sum", C.c_float * 3), ("hit_frames", C.c_uint32), ("sumsq", C.c_float * 3), ("frames", C.c_uint32)]


class TileState(C.Structure):
    """RtxTileState: the frames an 8 x 8 tile of the rectangle received and its noise estimate after its last add."""
    _fields_ = [("frames", C.c_uint32), ("err", C.c_float)]


class AdaptRule(C.Structure):
    """RtxAdaptRule: a tile is stopped when frames >= min_frames and err <= max_variance."""
    _fields_ = [("min_frames", C.c_uint32), ("max_variance", C.c_float)]


# the same bytes as numpy records: what moment_add works on
MOMENT_PIXEL_DTYPE = np.dtype([("sum", np.float32, 3), ("hit_frames", np.uint32), ("sumsq", np.float32, 3), ("frames", np.uint32)])
TILE_STATE_DTYPE = np.dtype([("frames", np.uint32), ("err", np.float32)])
assert MOMENT_PIXEL_DTYPE.itemsize == C.sizeof(MomentPixel) == 32 and TILE_STATE_DTYPE.itemsize == C.sizeof(TileState) == 8
ROWS_POSED = 1


class RtxView(C.Structure):
    """RtxView: a pinhole view of an uploaded scene (frame, camera after Camera::new) and the rectangle of it to render."""
    _fields_ = [("width", C.c_uint32), ("height", C.c_uint32),
                ("eye", C.c_float * 3), ("u", C.c_float * 3), ("v", C.c_float * 3), ("w", C.c_float * 3),
                ("distance", C.c_float),
                ("x0", C.c_uint32), ("y0", C.c_uint32), ("nx", C.c_uint32), ("ny", C.c_uint32)]


assert C.sizeof(RtxView) == 76 and C.alignment(RtxView) == 4


class RtxLight(C.Structure):
    """RtxLight: the area light of one lit call — Light.primitives[0]'s vertices and NB_LIGHT_SAMPLE (0 = the scene's)."""
    _fields_ = [("v0", C.c_float * 3), ("v1", C.c_float * 3), ("v2", C.c_float * 3), ("nb_light_sample", C.c_uint32)]


assert C.sizeof(RtxLight) == 40 and C.alignment(RtxLight) == 4


class RtxPosePrims(C.Structure):
    """RtxPosePrims: what a pose of every field states — host pointers for rtx_scene_pose_prims, device ones for _device."""
    _fields_ = [("v0v1v2", C.c_void_p), ("spheres", C.c_void_p), ("rgb", C.c_void_p), ("sphere_rgb", C.c_void_p),
                ("tie_rank", C.c_void_p)]


assert C.sizeof(RtxPosePrims) == 40 and C.alignment(RtxPosePrims) == 8
POSE_REBUILT = 1


class RtxPoseMoves(C.Structure):
    """RtxPoseMoves: the moves of a pose the device makes from the scene's geometry as created — host pointers for
    rtx_scene_pose_moved, device ones for _device."""
    _fields_ = [("n_moves", C.c_uint32), ("moves", C.c_void_p), ("group", C.c_void_p), ("radius_scale", C.c_void_p),
                ("rgb", C.c_void_p), ("sphere_rgb", C.c_void_p), ("tie_rank", C.c_void_p)]


assert C.sizeof(RtxPoseMoves) == 56 and C.alignment(RtxPoseMoves) == 8
MOVE_NONE = 0xFFFFFFFF
MAX_MOVES = 65536


class RtxSkin(C.Structure):
    """RtxSkin: the skin rtx_scene_skin binds to a scene — host pointers, copied by the call."""
    _fields_ = [("bones", C.c_void_p), ("weights", C.c_void_p), ("sphere_bone", C.c_void_p)]


assert C.sizeof(RtxSkin) == 24 and C.alignment(RtxSkin) == 8


# every symbol include/rtx.h declares (tests check the export list against the header)
_SIGS = {
    "rtx_abi_version": (C.c_int, []),
    "rtx_device_count": (C.c_int, []),
    "rtx_scene_create": (C.c_int, [C.POINTER(SceneDesc), C.POINTER(C.c_void_p)]),
    "rtx_scene_destroy": (None, [C.c_void_p]),
    "rtx_scene_info": (C.c_int, [C.c_void_p, C.POINTER(SceneInfo)]),
    "rtx_scene_upload": (C.c_int, [C.c_void_p, C.c_int]),
    "rtx_render_rows": (C.c_int, [C.c_void_p, C.c_int, C.c_uint32, C.c_uint32, C.c_void_p, C.POINTER(Stats)]),
    "rtx_render_frame": (C.c_int, [C.c_void_p, C.POINTER(C.c_int), C.c_int, C.c_uint32, C.c_void_p, C.POINTER(Stats)]),
    "rtx_render_tiles_device": (C.c_int, [C.c_void_p, C.c_int, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p,
                                          C.c_size_t, C.c_void_p, C.c_void_p]),
    "rtx_tiles_rows": (C.c_uint32, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32]),
    "rtx_tiles_bytes": (C.c_size_t, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32]),
    "rtx_trace_rays": (C.c_int, [C.c_void_p, C.c_int, C.c_uint32, f32p, f32p, C.c_uint32, C.POINTER(RayHit), C.POINTER(Stats)]),
    "rtx_occluded_rays": (C.c_int, [C.c_void_p, C.c_int, C.c_uint32, f32p, f32p, C.c_uint32, u8p, C.POINTER(Stats)]),
    "rtx_trace_rays_device": (C.c_int, [C.c_void_p, C.c_int, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]),
    "rtx_occluded_rays_device": (C.c_int, [C.c_void_p, C.c_int, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]),
    "rtx_shade_rays": (C.c_int, [C.c_void_p, C.c_int, C.c_uint32, f32p, f32p, C.c_uint32, C.POINTER(PixelShade),
                                 C.POINTER(RayHit), C.POINTER(Stats)]),
    "rtx_shade_rays_device": (C.c_int, [C.c_void_p, C.c_int, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p,
                                        C.c_void_p, C.c_void_p]),
    "rtx_scene_view": (C.c_int, [C.c_void_p, C.POINTER(RtxView)]),
    "rtx_render_view": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(RtxView), C.c_void_p, C.POINTER(PixelShade), C.POINTER(RayHit),
                                  C.POINTER(Stats)]),
    "rtx_render_view_device": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(RtxView), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "rtx_render_view_rows": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(RtxView), C.c_void_p, C.POINTER(Stats)]),
    "rtx_render_view_rows_device": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(RtxView), C.c_void_p, C.c_size_t, C.c_void_p,
                                              C.c_void_p]),
    "rtx_scene_aimed_nodes": (C.c_int, [C.c_void_p, f32p, u32p]),
    "rtx_debug_aimed_nodes": (C.c_int, [C.c_void_p, C.c_int, f32p, u32p]),
    "rtx_scene_light": (C.c_int, [C.c_void_p, C.POINTER(RtxLight)]),
    "rtx_scene_light_points_for": (C.c_int, [C.c_void_p, C.POINTER(RtxLight), f32p]),
    "rtx_debug_light_points": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(RtxLight), f32p]),
    "rtx_render_view_rows_lit": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(RtxView), C.POINTER(RtxLight), C.c_void_p,
                                           C.POINTER(Stats)]),
    "rtx_render_view_rows_lit_device": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(RtxView), C.POINTER(RtxLight), C.c_void_p,
                                                  C.c_size_t, C.c_void_p, C.c_void_p]),
    "rtx_scene_light_walk_for": (C.c_int, [C.c_void_p, C.POINTER(RtxLight), u32p, f32p, f32p]),
    "rtx_debug_light_walk": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(RtxLight), f32p, f32p]),
    "rtx_render_view_lit": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(RtxView), C.POINTER(RtxLight), C.c_void_p,
                                      C.POINTER(PixelShade), C.POINTER(RayHit), C.POINTER(Stats)]),
    "rtx_render_view_lit_device": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(RtxView), C.POINTER(RtxLight), C.c_void_p, C.c_void_p,
                                             C.c_void_p, C.c_void_p]),
    "rtx_shade_rays_lit": (C.c_int, [C.c_void_p, C.c_int, C.c_uint32, f32p, f32p, C.c_uint32, C.POINTER(RtxLight),
                                     C.POINTER(PixelShade), C.POINTER(RayHit), C.POINTER(Stats)]),
    "rtx_shade_rays_lit_device": (C.c_int, [C.c_void_p, C.c_int, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32,
                                            C.POINTER(RtxLight), C.c_void_p, C.c_void_p, C.c_void_p]),
    "rtx_scene_pose_bound": (C.c_int, [C.c_void_p, f32p]),
    "rtx_scene_pose": (C.c_int, [C.c_void_p, C.c_int, f32p, u32p, C.c_uint32, C.POINTER(Stats)]),
    "rtx_scene_pose_device": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "rtx_scene_posed_records": (C.c_int, [C.c_void_p, f32p, u32p, u32p, u32p, u32p]),
    "rtx_debug_pose": (C.c_int, [C.c_void_p, C.c_int, u32p, u32p, u32p]),
    "rtx_trace_rays_posed": (C.c_int, [C.c_void_p, C.c_int, C.c_uint32, f32p, f32p, C.c_uint32, C.POINTER(RayHit), C.POINTER(Stats)]),
    "rtx_occluded_rays_posed": (C.c_int, [C.c_void_p, C.c_int, C.c_uint32, f32p, f32p, C.c_uint32, u8p, C.POINTER(Stats)]),
    "rtx_trace_rays_posed_device": (C.c_int, [C.c_void_p, C.c_int, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p,
                                              C.c_void_p]),
    "rtx_occluded_rays_posed_device": (C.c_int, [C.c_void_p, C.c_int, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p,
                                                 C.c_void_p]),
    "rtx_shade_rays_posed": (C.c_int, [C.c_void_p, C.c_int, C.c_uint32, f32p, f32p, C.c_uint32, C.POINTER(RtxLight),
                                       C.POINTER(PixelShade), C.POINTER(RayHit), C.POINTER(Stats)]),
    "rtx_shade_rays_posed_device": (C.c_int, [C.c_void_p, C.c_int, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32,
                                              C.POINTER(RtxLight), C.c_void_p, C.c_void_p, C.c_void_p]),
    "rtx_render_view_posed": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(RtxView), C.POINTER(RtxLight), C.c_void_p,
                                        C.POINTER(PixelShade), C.POINTER(RayHit), C.POINTER(Stats)]),
    "rtx_render_view_posed_device": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(RtxView), C.POINTER(RtxLight), C.c_void_p, C.c_void_p,
                                               C.c_void_p, C.c_void_p]),
    "rtx_render_view_rows_posed": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(RtxView), C.POINTER(RtxLight), C.c_void_p,
                                             C.POINTER(Stats)]),
    "rtx_render_view_rows_posed_device": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(RtxView), C.POINTER(RtxLight), C.c_void_p,
                                                    C.c_size_t, C.c_void_p, C.c_void_p]),
    "rtx_render_view_rows_shade": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(RtxView), C.POINTER(RtxLight), C.c_uint32,
                                             C.POINTER(PixelShade), C.POINTER(Stats)]),
    "rtx_render_view_rows_shade_device": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(RtxView), C.POINTER(RtxLight), C.c_uint32,
                                                    C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]),
    "rtx_scene_posed_pipeline_records": (C.c_int, [C.c_void_p, f32p, f32p, u32p, u32p]),
    "rtx_debug_pose_pipeline": (C.c_int, [C.c_void_p, C.c_int, f32p, u32p, u32p]),
    "rtx_scene_pose_rebuilt": (C.c_int, [C.c_void_p, C.c_int, f32p, u32p, C.c_uint32, C.POINTER(Stats)]),
    "rtx_scene_pose_rebuilt_device": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "rtx_scene_rebuilt_counts": (C.c_int, [C.c_void_p, u32p]),
    "rtx_scene_rebuilt_records": (C.c_int, [C.c_void_p, f32p, u32p, C.POINTER(C.c_uint64), u32p, u32p, u32p, u32p]),
    "rtx_scene_rebuilt_aimed": (C.c_int, [C.c_void_p, f32p, f32p, u32p]),
    "rtx_debug_pose_rebuilt": (C.c_int, [C.c_void_p, C.c_int, f32p, u32p, u32p, u32p, u32p, u32p]),
    "rtx_scene_pose_prims": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(RtxPosePrims), C.c_uint32, C.c_uint32, C.POINTER(Stats)]),
    "rtx_scene_pose_prims_device": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(RtxPosePrims), C.c_uint32, C.c_void_p]),
    "rtx_scene_pose_prims_records": (C.c_int, [C.c_void_p, C.POINTER(RtxPosePrims), C.c_uint32, C.POINTER(C.c_uint64), u32p, u32p,
                                              u32p, u32p]),
    "rtx_scene_pose_prims_aimed": (C.c_int, [C.c_void_p, C.POINTER(RtxPosePrims), C.c_uint32, f32p, u32p]),
    "rtx_scene_pose_moved": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(RtxPoseMoves), C.c_uint32, C.c_uint32, C.POINTER(Stats)]),
    "rtx_scene_pose_moved_device": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(RtxPoseMoves), C.c_uint32, C.c_void_p]),
    "rtx_scene_moved_prims": (C.c_int, [C.c_void_p, C.POINTER(RtxPoseMoves), f32p, f32p]),
    "rtx_debug_moved_prims": (C.c_int, [C.c_void_p, C.c_int, f32p, f32p]),
    "rtx_scene_skin": (C.c_int, [C.c_void_p, C.POINTER(RtxSkin)]),
    "rtx_scene_skin_bound": (C.c_int, [C.c_void_p, u32p]),
    "rtx_scene_pose_skinned": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(RtxPoseMoves), C.c_uint32, C.c_uint32, C.POINTER(Stats)]),
    "rtx_scene_pose_skinned_device": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(RtxPoseMoves), C.c_uint32, C.c_void_p]),
    "rtx_scene_skinned_prims": (C.c_int, [C.c_void_p, C.POINTER(RtxPoseMoves), f32p, f32p]),
    "rtx_scene_resample": (C.c_int, [C.c_void_p, f32p, C.c_uint32]),
    "rtx_scene_reseed": (C.c_int, [C.c_void_p, C.c_uint64, C.c_uint32]),
    "rtx_scene_samples": (C.c_int, [C.c_void_p, C.c_uint64, C.c_uint32, f32p]),
    "rtx_debug_samples": (C.c_int, [C.c_void_p, C.c_int, C.c_uint64, C.c_uint32, f32p]),
    "rtxh_accum_add": (C.c_int, [C.c_uint32, C.POINTER(PixelShade), C.POINTER(AccumPixel), C.c_uint32]),
    "rtxh_accum_resolve": (C.c_int, [f32p, C.c_uint32, C.POINTER(AccumPixel), C.c_uint32, C.c_void_p, C.POINTER(PixelShade)]),
    "rtx_accum_add_device": (C.c_int, [C.c_void_p, C.c_int, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]),
    "rtx_accum_resolve_device": (C.c_int, [C.c_void_p, C.c_int, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p,
                                           C.c_void_p]),
    "rtx_render_view_mean": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(RtxView), C.POINTER(RtxLight), C.c_uint32, u64p, C.c_uint32,
                                       C.c_uint32, C.c_void_p, C.POINTER(PixelShade), C.POINTER(Stats)]),
    "rtx_render_view_mean_device": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(RtxView), C.POINTER(RtxLight), C.c_uint32, u64p,
                                              C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "rtxh_moment_add": (C.c_int, [C.c_uint32, C.c_uint32, C.POINTER(PixelShade), C.POINTER(MomentPixel), C.POINTER(TileState), C.c_uint32,
                                  C.POINTER(AdaptRule)]),
    "rtxh_moment_resolve": (C.c_int, [f32p, C.c_uint32, C.POINTER(MomentPixel), C.c_void_p, C.POINTER(PixelShade)]),
    "rtx_moment_add_device": (C.c_int, [C.c_void_p, C.c_int, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32,
                                        C.POINTER(AdaptRule), C.c_void_p]),
    "rtx_moment_resolve_device": (C.c_int, [C.c_void_p, C.c_int, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "rtx_render_view_adaptive": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(RtxView), C.POINTER(RtxLight), C.c_uint32, u64p, C.c_uint32,
                                           C.c_uint32, C.POINTER(AdaptRule), C.c_void_p, C.POINTER(PixelShade), C.POINTER(TileState),
                                           C.POINTER(Stats)]),
    "rtx_render_view_adaptive_device": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(RtxView), C.POINTER(RtxLight), C.c_uint32, u64p,
                                                  C.c_uint32, C.c_uint32, C.POINTER(AdaptRule), C.c_void_p, C.c_void_p, C.c_void_p,
                                                  C.c_void_p, C.c_void_p]),
    "rtx_render_view_rows_mean": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(RtxView), C.POINTER(RtxLight), C.c_uint32, u64p, C.c_uint32,
                                            C.c_uint32, C.c_void_p, C.POINTER(PixelShade), C.POINTER(Stats)]),
    "rtx_render_view_rows_mean_device": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(RtxView), C.POINTER(RtxLight), C.c_uint32, u64p,
                                                   C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "rtx_render_view_rows_adaptive": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(RtxView), C.POINTER(RtxLight), C.c_uint32, u64p,
                                                C.c_uint32, C.c_uint32, C.POINTER(AdaptRule), C.c_void_p, C.POINTER(PixelShade),
                                                C.POINTER(TileState), C.POINTER(Stats)]),
    "rtx_render_view_rows_adaptive_device": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(RtxView), C.POINTER(RtxLight), C.c_uint32, u64p,
                                                       C.c_uint32, C.c_uint32, C.POINTER(AdaptRule), C.c_void_p, C.c_void_p, C.c_void_p,
                                                       C.c_void_p, C.c_void_p]),
    "rtx_render_view_rows_shade_masked_device": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(RtxView), C.POINTER(RtxLight), C.c_uint32,
                                                           C.c_void_p, C.POINTER(AdaptRule), C.c_void_p, C.c_size_t, C.c_void_p,
                                                           C.c_void_p]),
    "rtx_scene_light_walk_seeded": (C.c_int, [C.c_void_p, C.POINTER(RtxLight), C.c_uint64, C.c_uint32, u32p, f32p, f32p]),
    "rtx_debug_wave_profile": (C.c_int, [C.c_void_p, C.c_int, C.c_uint32, C.c_uint32, u64p, C.c_size_t, u32p, u32p]),
    "rtx_launch_timings": (C.c_int, [C.c_void_p, C.c_int, C.c_int, f32p, f32p]),
    "rtx_debug_tile_descs": (C.c_int, [C.c_void_p, C.c_int, u32p, C.c_size_t]),
    "rtx_debug_probe_records": (C.c_int, [C.c_void_p, C.c_int, u32p, u32p, C.c_size_t]),
    "rtx_scene_probe_long": (C.c_int, [C.c_void_p, u32p, u32p, C.c_size_t, u32p]),
    "rtx_scene_probe_tile": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, u8p, u32p]),
    "rtx_debug_probe_split": (C.c_int, [C.c_void_p, C.c_uint32]),
    "rtx_strerror": (C.c_char_p, [C.c_int]),
    "rtx_last_hip_error": (C.c_int, []),
    "rtx_scene_light_points": (C.c_int, [C.c_void_p, f32p]),
    "rtx_scene_light_order": (C.c_int, [C.c_void_p, u32p]),
    "rtx_scene_gamma_thresholds": (C.c_int, [C.c_void_p, f32p]),
    "rtx_scene_normals": (C.c_int, [C.c_void_p, f32p]),
    "rtx_scene_nodes": (C.c_int, [C.c_void_p, u32p, u32p]),
    "rtx_scene_primary_nodes": (C.c_int, [C.c_void_p, u32p, u32p]),
    "rtx_scene_ref_nodes": (C.c_int, [C.c_void_p, u32p]),
    "rtxh_camera_new": (None, [f32p] * 6),
    "rtxh_import_obj": (C.c_int, [C.c_char_p, C.POINTER(f32p)]),
    "rtxh_import_obj_ex": (C.c_int, [C.c_char_p, C.c_uint32, C.POINTER(f32p), C.POINTER(f32p)]),
    "rtxh_free": (None, [C.c_void_p]),
    "rtxh_ref_leaf_rank": (C.c_int, [C.c_uint32, f32p, u32p]),
    "rtxh_gen_samples": (None, [C.c_uint64, C.c_uint32, f32p]),
    "rtxh_write_png": (C.c_int, [C.c_char_p, C.c_uint32, C.c_uint32, C.c_void_p]),
    "rtxh_synthetic_mesh": (C.c_int, [C.c_uint64, C.c_uint32, f32p]),
    "rtxh_scatter_tiles": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32]),
}
for _name, (_res, _args) in _SIGS.items():
    _fn = getattr(_lib, _name)
    _fn.restype = _res
    _fn.argtypes = _args


class RtxError(RuntimeError):
    def __init__(self, code, where=""):
        self.code = code
        msg = _lib.rtx_strerror(code).decode()
        if code == ERR_HIP:
            msg += " (hipError %d)" % _lib.rtx_last_hip_error()
        super().__init__("%s: %s [%d]" % (where, msg, code))


def _check(code, where):
    if code != OK:
        raise RtxError(code, where)


def _fp(a):
    return a.ctypes.data_as(f32p)


def _up(a):
    """uint32 words of an array, None: NULL"""
    return a.ctypes.data_as(u32p) if a is not None else None


def _f3(x):
    return np.ascontiguousarray(np.asarray(x, dtype=np.float32).reshape(3))


def abi_version():
    return _lib.rtx_abi_version()


def device_count():
    return _lib.rtx_device_count()


# ------------------------------------------------------------------ host helpers (rtxh_*)
def camera_new(eye, look_at, up):
    """Camera::new (src/tracer/utils/camera.rs:17-35) -> (u, v, w)."""
    u, v, w = (np.zeros(3, np.float32) for _ in range(3))
    _lib.rtxh_camera_new(_fp(_f3(eye)), _fp(_f3(look_at)), _fp(_f3(up)), _fp(u), _fp(v), _fp(w))
    return u, v, w


def import_obj(path):
    """import_obj (src/main.rs:114-149) -> float32 [n, 9] (v0, v1, v2 per triangle)."""
    p = f32p()
    n = _lib.rtxh_import_obj(os.fsencode(path), C.byref(p))
    if n < 0:
        raise RtxError(n, "rtxh_import_obj(%s)" % path)
    arr = np.ctypeslib.as_array(p, shape=(max(n, 1), 9))[:n].copy() if n else np.zeros((0, 9), np.float32)
    _lib.rtxh_free(p)
    return arr


OBJ_SLASHES, OBJ_RELATIVE, OBJ_POLYGONS, OBJ_MATERIALS, OBJ_ALL = 1, 2, 4, 8, 15


def import_obj_ex(path, flags=OBJ_ALL):
    """The loader with slashes, relative indices, polygons and material colours (each opt-in; flags = 0 is
    import_obj with every triangle white) -> (float32 [n, 9], float32 [n, 3])."""
    t, c = f32p(), f32p()
    n = _lib.rtxh_import_obj_ex(os.fsencode(path), flags, C.byref(t), C.byref(c))
    if n < 0:
        raise RtxError(n, "rtxh_import_obj_ex(%s)" % path)
    tris = np.ctypeslib.as_array(t, shape=(max(n, 1), 9))[:n].copy() if n else np.zeros((0, 9), np.float32)
    rgb = np.ctypeslib.as_array(c, shape=(max(n, 1), 3))[:n].copy() if n else np.zeros((0, 3), np.float32)
    _lib.rtxh_free(t)
    _lib.rtxh_free(c)
    return tris, rgb


def ref_leaf_rank(tris):
    tris = np.ascontiguousarray(tris, dtype=np.float32).reshape(-1, 9)
    out = np.zeros(len(tris), dtype=np.uint32)
    _check(_lib.rtxh_ref_leaf_rank(len(tris), _fp(tris), out.ctypes.data_as(u32p)), "rtxh_ref_leaf_rank")
    return out


def gen_samples(seed=DEFAULT_SEED, n_pairs=NB_RAND_SAMPLE):
    out = np.empty((n_pairs, 2), dtype=np.float32)
    _lib.rtxh_gen_samples(seed, n_pairs, _fp(out))
    return out


def accum_add(shade, accum=None):
    """Host only: the accumulator statement over arrays (rtxh_accum_add).  shade: PIXEL_SHADE_DTYPE records of one frame;
    accum: ACCUM_PIXEL_DTYPE records of the same shape, updated in place and returned — None: the first frame, a new array
    whose old content is never read."""
    s = np.ascontiguousarray(shade, dtype=PIXEL_SHADE_DTYPE)
    first = accum is None
    if first:
        accum = np.empty(s.shape, ACCUM_PIXEL_DTYPE)
    assert accum.dtype == ACCUM_PIXEL_DTYPE and accum.flags["C_CONTIGUOUS"] and accum.size == s.size
    _check(_lib.rtxh_accum_add(s.size, s.ctypes.data_as(C.POINTER(PixelShade)), accum.ctypes.data_as(C.POINTER(AccumPixel)),
                               1 if first else 0), "rtxh_accum_add")
    return accum


def accum_resolve(thresholds, accum, n_frames):
    """Host only: the resolve statement over arrays (rtxh_accum_resolve) -> (uint8 [..., 3], PIXEL_SHADE_DTYPE records);
    thresholds: a scene's 256 (Scene.gamma_thresholds)."""
    thr = np.ascontiguousarray(thresholds, dtype=np.float32)
    a = np.ascontiguousarray(accum, dtype=ACCUM_PIXEL_DTYPE)
    assert thr.size == 256
    rgb, shade = np.zeros(a.shape + (3,), np.uint8), np.zeros(a.shape, PIXEL_SHADE_DTYPE)
    _check(_lib.rtxh_accum_resolve(_fp(thr), a.size, a.ctypes.data_as(C.POINTER(AccumPixel)), int(n_frames), rgb.ctypes.data,
                                   shade.ctypes.data_as(C.POINTER(PixelShade))), "rtxh_accum_resolve")
    return rgb, shade


def tile_grid(nx, ny):
    """(tiles_x, tiles_y) of an nx x ny rectangle: its 8 x 8 tiles, row by row"""
    return (nx + 7) // 8, (ny + 7) // 8


def moment_add(shade, moments=None, tiles=None, rule=None):
    """Host only: the adaptive mean's add over a rectangle (rtxh_moment_add).  shade: PIXEL_SHADE_DTYPE records [ny, nx] of one
    frame; moments: MOMENT_PIXEL_DTYPE [ny, nx], updated in place and returned — None: the first frame, new arrays whose old
    content is never read.  rule: None (no tile states: the plain moment accumulator -> moments) or (min_frames,
    max_variance) -> (moments, tiles), tiles TILE_STATE_DTYPE [tiles_y, tiles_x], updated in place when given."""
    s = np.ascontiguousarray(shade, dtype=PIXEL_SHADE_DTYPE)
    assert s.ndim == 2
    ny, nx = s.shape
    first = moments is None
    if first:
        moments = np.empty(s.shape, MOMENT_PIXEL_DTYPE)
        assert tiles is None
    assert moments.dtype == MOMENT_PIXEL_DTYPE and moments.flags["C_CONTIGUOUS"] and moments.shape == s.shape
    r = None
    if rule is not None:
        r = AdaptRule(int(rule[0]), float(rule[1]))
        if tiles is None:
            assert first
            tiles = np.empty(tile_grid(nx, ny)[::-1], TILE_STATE_DTYPE)
        assert tiles.dtype == TILE_STATE_DTYPE and tiles.flags["C_CONTIGUOUS"] and tiles.shape == tile_grid(nx, ny)[::-1]
    _check(_lib.rtxh_moment_add(nx, ny, s.ctypes.data_as(C.POINTER(PixelShade)), moments.ctypes.data_as(C.POINTER(MomentPixel)),
                                tiles.ctypes.data_as(C.POINTER(TileState)) if rule is not None else None, 1 if first else 0,
                                C.byref(r) if r is not None else None), "rtxh_moment_add")
    return moments if rule is None else (moments, tiles)


def moment_resolve(thresholds, moments):
    """Host only: the adaptive mean's resolve over arrays (rtxh_moment_resolve) -> (uint8 [..., 3], PIXEL_SHADE_DTYPE records):
    every pixel divided by its own frame count; thresholds: a scene's 256 (Scene.gamma_thresholds)."""
    thr = np.ascontiguousarray(thresholds, dtype=np.float32)
    m = np.ascontiguousarray(moments, dtype=MOMENT_PIXEL_DTYPE)
    assert thr.size == 256
    rgb, shade = np.zeros(m.shape + (3,), np.uint8), np.zeros(m.shape, PIXEL_SHADE_DTYPE)
    _check(_lib.rtxh_moment_resolve(_fp(thr), m.size, m.ctypes.data_as(C.POINTER(MomentPixel)), rgb.ctypes.data,
                                    shade.ctypes.data_as(C.POINTER(PixelShade))), "rtxh_moment_resolve")
    return rgb, shade


def write_png(path, img):
    img = np.ascontiguousarray(img, dtype=np.uint8)
    h, w, c = img.shape
    assert c == 3
    _check(_lib.rtxh_write_png(os.fsencode(path), w, h, img.ctypes.data), "rtxh_write_png")


SYNTHETIC_SEED = 12345


def synthetic_mesh(n_tris, seed=SYNTHETIC_SEED):
    """BASELINE.json configs[4]: random triangle soup in the big_bunny AABB -> float32 [n, 9]."""
    out = np.empty((n_tris, 9), dtype=np.float32)
    _check(_lib.rtxh_synthetic_mesh(seed, n_tris, _fp(out)), "rtxh_synthetic_mesh")
    return out


def synthetic_primitives(n_tris, seed=SYNTHETIC_SEED):
    """Synthetic soup (colour 1,1,1) + the ground, ground last as in main() (src/main.rs:335)."""
    t = synthetic_mesh(n_tris, seed)
    tris = np.concatenate([t, np.asarray(GROUND_TRI, np.float32).reshape(1, 9)])
    rgb = np.concatenate([np.tile(np.asarray(MESH_RGB, np.float32), (n_tris, 1)),
                          np.asarray(GROUND_RGB, np.float32).reshape(1, 3)])
    return np.ascontiguousarray(tris), np.ascontiguousarray(rgb)


def default_primitives(obj_paths):
    """The primitive list main() builds: OBJ meshes in argv order, ground last (src/main.rs:327-335)."""
    parts, cols = [], []
    for p in obj_paths:
        t = import_obj(p)
        parts.append(t)
        cols.append(np.tile(np.asarray(MESH_RGB, np.float32), (len(t), 1)))
    parts.append(np.asarray(GROUND_TRI, np.float32).reshape(1, 9))
    cols.append(np.asarray(GROUND_RGB, np.float32).reshape(1, 3))
    return np.ascontiguousarray(np.concatenate(parts)), np.ascontiguousarray(np.concatenate(cols))


# ------------------------------------------------------------------ Scene
class Scene:
    """Flattened Scene{width,height,light,camera,bvh}; owns an RtxScene handle."""

    def __init__(self, width, height, tris, rgb, samples, *, eye=DEFAULT_EYE, look_at=DEFAULT_LOOK_AT,
                 up=DEFAULT_UP, distance=DEFAULT_DISTANCE, light_tri=DEFAULT_LIGHT, nb_ray=NB_RAY,
                 nb_light_sample=NB_LIGHT_SAMPLE, accel=ACCEL_BVH, leaf_max=0, tie_rank="reference",
                 reference_tree=REFTREE_AUTO, spheres=None, sphere_rgb=None, kinds=None):
        """spheres [m, 4] (origin x, y, z, radius) and sphere_rgb [m, 3] are the Sphere arm of Primitive
        (src/tracer/primitives/sphere.rs:12-29); kinds (uint8 per primitive, 0 = next triangle, 1 = next sphere)
        gives the order of the Vec<Primitive>, default all triangles then all spheres.  tie_rank, when given,
        is indexed by position in that Vec."""
        self._h = C.c_void_p()
        self.width, self.height = int(width), int(height)
        self.tris = np.ascontiguousarray(tris, dtype=np.float32).reshape(-1, 9)
        self.rgb = np.ascontiguousarray(rgb, dtype=np.float32).reshape(-1, 3)
        self.samples = np.ascontiguousarray(samples, dtype=np.float32).reshape(-1, 2)
        if len(self.rgb) != len(self.tris):
            raise ValueError("rgb and tris disagree")
        self.spheres = np.zeros((0, 4), np.float32) if spheres is None else \
            np.ascontiguousarray(spheres, dtype=np.float32).reshape(-1, 4)
        self.sphere_rgb = np.ones((len(self.spheres), 3), np.float32) if sphere_rgb is None else \
            np.ascontiguousarray(sphere_rgb, dtype=np.float32).reshape(-1, 3)
        if len(self.sphere_rgb) != len(self.spheres):
            raise ValueError("sphere_rgb and spheres disagree")
        self.kinds = None if kinds is None else np.ascontiguousarray(kinds, dtype=np.uint8).reshape(-1)
        if self.kinds is not None and len(self.kinds) != len(self.tris) + len(self.spheres):
            raise ValueError("kinds must have one entry per primitive")
        self.n_prims = len(self.tris) + len(self.spheres)
        self.nb_ray = int(nb_ray)
        if isinstance(tie_rank, str):
            if tie_rank != "reference":
                raise ValueError(tie_rank)
            rank = None          # the library derives it from the reference tree it builds (reference_tree)
        else:
            rank = None if tie_rank is None else np.ascontiguousarray(tie_rank, dtype=np.uint32)
            if tie_rank is None and reference_tree == REFTREE_AUTO:
                reference_tree = REFTREE_NEVER   # tie_rank=None means "index order, no reference tree"
        self.tie_rank = rank
        u, v, w = camera_new(eye, look_at, up)
        lt = np.asarray(light_tri, dtype=np.float32).reshape(9)
        d = SceneDesc()
        d.width, d.height = self.width, self.height
        d.eye[:] = _f3(eye).tolist()
        d.u[:], d.v[:], d.w[:] = u.tolist(), v.tolist(), w.tolist()
        d.distance = float(distance)
        d.light_v0[:], d.light_v1[:], d.light_v2[:] = lt[0:3].tolist(), lt[3:6].tolist(), lt[6:9].tolist()
        d.n_tris = len(self.tris)
        d.v0v1v2, d.rgb = _fp(self.tris), _fp(self.rgb)
        d.n_spheres = len(self.spheres)
        if len(self.spheres):
            d.spheres, d.sphere_rgb = _fp(self.spheres), _fp(self.sphere_rgb)
        if self.kinds is not None:
            d.kinds = self.kinds.ctypes.data_as(u8p)
        if rank is not None and len(rank) != self.n_prims:
            raise ValueError("tie_rank must have one entry per primitive")
        d.tie_rank = rank.ctypes.data_as(u32p) if rank is not None else None
        d.nb_ray, d.nb_light_sample = int(nb_ray), int(nb_light_sample)
        d.samples, d.n_samples = _fp(self.samples), len(self.samples)
        d.accel, d.leaf_max, d.reference_tree = int(accel), int(leaf_max), int(reference_tree)
        _check(_lib.rtx_scene_create(C.byref(d), C.byref(self._h)), "rtx_scene_create")

    # -- lifetime
    def close(self):
        if self._h:
            _lib.rtx_scene_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    @property
    def handle(self):
        return self._h

    # -- prepared-scene read-back
    def info(self):
        i = SceneInfo()
        _check(_lib.rtx_scene_info(self._h, C.byref(i)), "rtx_scene_info")
        return i.asdict()

    def light_points(self):
        n = self.info()["n_light_points"]
        out = np.zeros((n, 3), np.float32)
        _check(_lib.rtx_scene_light_points(self._h, _fp(out)), "rtx_scene_light_points")
        return out

    def light_order(self):
        """-> (nb_ray, nb_light_sample) sample indices in the order the shading pass walks them, batch after batch"""
        out = np.zeros(self.info()["n_light_points"], np.uint32)
        if len(out):
            _check(_lib.rtx_scene_light_order(self._h, out.ctypes.data_as(u32p)), "rtx_scene_light_order")
        return out

    def gamma_thresholds(self):
        out = np.zeros(256, np.float32)
        _check(_lib.rtx_scene_gamma_thresholds(self._h, _fp(out)), "rtx_scene_gamma_thresholds")
        return out

    def normals(self):
        out = np.zeros((self.n_prims, 3), np.float32)      # a sphere's row holds its origin (its normal needs p_hit)
        _check(_lib.rtx_scene_normals(self._h, _fp(out)), "rtx_scene_normals")
        return out

    def nodes(self):
        i = self.info()
        nd = np.zeros((i["n_nodes"], 8), np.uint32)
        order = np.zeros(i["n_tris"], np.uint32)
        _check(_lib.rtx_scene_nodes(self._h, nd.ctypes.data_as(u32p), order.ctypes.data_as(u32p)), "rtx_scene_nodes")
        return nd, order

    def primary_nodes(self):
        """-> (records of the primary rays' stream, whether the scene has one of its own)"""
        nd = np.zeros((self.info()["n_nodes"], 8), np.uint32)
        own = C.c_uint32(0)
        _check(_lib.rtx_scene_primary_nodes(self._h, nd.ctypes.data_as(u32p), C.cast(C.byref(own), u32p)), "rtx_scene_primary_nodes")
        return nd, bool(own.value)

    def ref_nodes(self):
        nd = np.zeros((self.info()["n_ref_nodes"], 8), np.uint32)
        if len(nd):
            _check(_lib.rtx_scene_ref_nodes(self._h, nd.ctypes.data_as(u32p)), "rtx_scene_ref_nodes")
        return nd

    # -- rendering (GPU only)
    def upload(self, device=0):
        _check(_lib.rtx_scene_upload(self._h, device), "rtx_scene_upload")

    def render_rows(self, row0=0, nrows=None, device=0, stats=False, out_ptr=None):
        """out_ptr: address of a caller-owned host buffer of nrows*width*3 bytes (e.g. pinned memory) to render into
        instead of a fresh numpy array; the call then returns None (or the statistics)."""
        if nrows is None:
            nrows = self.height - row0
        out = None if out_ptr else np.zeros((nrows, self.width, 3), np.uint8)
        st = Stats()
        _check(_lib.rtx_render_rows(self._h, device, row0, nrows, C.c_void_p(out_ptr) if out_ptr else out.ctypes.data,
                                    C.byref(st) if stats else None), "rtx_render_rows")
        if out_ptr:
            return st.asdict() if stats else None
        return (out, st.asdict()) if stats else out

    def render_frame(self, devices=(0,), tile_rows=8, stats=False):
        out = np.zeros((self.height, self.width, 3), np.uint8)
        devs = (C.c_int * len(devices))(*devices)
        st = Stats()
        _check(_lib.rtx_render_frame(self._h, devs, len(devices), tile_rows, out.ctypes.data,
                                     C.byref(st) if stats else None), "rtx_render_frame")
        return (out, st.asdict()) if stats else out

    def wave_profile(self, row0=0, nrows=None, device=0):
        """Diagnostics: [tiles_y, tiles_x, 8] uint64 {node fetches, triangle fetches, start, end, primary phase,
        shadow phase (slowest wavefront), accumulation phase, -}; times in 100 MHz ticks.  Ablation build only
        (RTX_PY_ABLATION=1): librtx.so answers ERR_UNSUPPORTED."""
        if nrows is None:
            nrows = self.height - row0
        tx, ty = C.c_uint32(), C.c_uint32()
        _check(_lib.rtx_debug_wave_profile(self._h, device, row0, nrows, None, 0, C.byref(tx), C.byref(ty)),
               "rtx_debug_wave_profile")
        out = np.zeros((ty.value, tx.value, 8), np.uint64)
        _check(_lib.rtx_debug_wave_profile(self._h, device, row0, nrows, out.ctypes.data_as(u64p), tx.value * ty.value,
                                           C.byref(tx), C.byref(ty)), "rtx_debug_wave_profile")
        return out

    def launch_timings(self, device=0, max_launches=64):
        """Device milliseconds of the most recent launches, oldest first: (scheduling pass, shading pass) arrays."""
        a = np.zeros(max_launches, np.float32)
        b = np.zeros(max_launches, np.float32)
        n = _lib.rtx_launch_timings(self._h, device, max_launches, _fp(a), _fp(b))
        if n < 0:
            raise RtxError(n, "rtx_launch_timings")
        return a[:n], b[:n]

    def tile_descs(self, device=0):
        """Diagnostics: uint32 [tiles, 4] {cost class, primary hits, flags, reserved} of the most recent launch."""
        n = _lib.rtx_debug_tile_descs(self._h, device, None, 0)
        if n < 0:
            raise RtxError(n, "rtx_debug_tile_descs")
        out = np.zeros((n, 4), np.uint32)
        m = _lib.rtx_debug_tile_descs(self._h, device, out.ctypes.data_as(u32p), n)
        if m < 0:
            raise RtxError(m, "rtx_debug_tile_descs")
        return out[:m]

    def probe_records(self, device=0):
        """Diagnostics: (hit words uint32 [tiles, 768], pixel slots uint32 [tiles, 64]) of the most recent launch's
        scheduling pass, in tile_descs' numbering."""
        n = _lib.rtx_debug_probe_records(self._h, device, None, None, 0)
        if n < 0:
            raise RtxError(n, "rtx_debug_probe_records")
        hits, slots = np.zeros((n, 768), np.uint32), np.zeros((n, 64), np.uint32)
        m = _lib.rtx_debug_probe_records(self._h, device, hits.ctypes.data_as(u32p), slots.ctypes.data_as(u32p), n)
        if m < 0:
            raise RtxError(m, "rtx_debug_probe_records")
        return hits[:m], slots[:m]

    def probe_long(self):
        """-> (long list: frame tile numbers costliest first, their weights, the threshold); host only."""
        n = _lib.rtx_scene_probe_long(self._h, None, None, 0, None)
        if n < 0:
            raise RtxError(n, "rtx_scene_probe_long")
        tiles, weights, thr = np.zeros(n, np.uint32), np.zeros(n, np.uint32), C.c_uint32(0)
        m = _lib.rtx_scene_probe_long(self._h, tiles.ctypes.data_as(u32p), weights.ctypes.data_as(u32p), n,
                                      C.cast(C.byref(thr), u32p))
        if m < 0:
            raise RtxError(m, "rtx_scene_probe_long")
        return tiles[:m], weights[:m], thr.value

    def probe_tile(self, tile_x, tile_y):
        """-> (weight, uint8 [n_nodes]: 1 where the tile's frustum meets the record of primary_nodes(), predicted?)"""
        met = np.zeros(self.info()["n_nodes"], np.uint8)
        w = C.c_uint32(0)
        rc = _lib.rtx_scene_probe_tile(self._h, tile_x, tile_y, met.ctypes.data_as(u8p), C.cast(C.byref(w), u32p))
        if rc < 0:
            raise RtxError(rc, "rtx_scene_probe_tile")
        return w.value, met, bool(rc)

    def debug_probe_split(self, mode):
        """0: the predicted long tiles (default), 1: none, 2: every tile -> long-list workgroups of the scene's most
        recent pipeline launch."""
        n = _lib.rtx_debug_probe_split(self._h, mode)
        if n < 0:
            raise RtxError(n, "rtx_debug_probe_split")
        return n

    def tiles_rows(self, first_tile, tile_stride, tile_rows):
        return _lib.rtx_tiles_rows(self._h, first_tile, tile_stride, tile_rows)

    def tiles_bytes(self, first_tile, tile_stride, tile_rows):
        return _lib.rtx_tiles_bytes(self._h, first_tile, tile_stride, tile_rows)

    def render_tiles_device(self, device, first_tile, tile_stride, tile_rows, d_out_ptr, d_out_bytes,
                            stream=None, d_counters_ptr=None):
        """Asynchronous launch into a device buffer the caller owns (e.g. a torch uint8 tensor)."""
        _check(_lib.rtx_render_tiles_device(self._h, device, first_tile, tile_stride, tile_rows,
                                            C.c_void_p(d_out_ptr), d_out_bytes,
                                            C.c_void_p(stream) if stream else None,
                                            C.c_void_p(d_counters_ptr) if d_counters_ptr else None),
               "rtx_render_tiles_device")

    # -- ray queries (GPU only): rays the caller supplies
    @staticmethod
    def _ray_flags(keep_order, force_regroup):
        return (RAYS_KEEP_ORDER if keep_order else 0) | (RAYS_FORCE_REGROUP if force_regroup else 0)

    @staticmethod
    def _ray_arrays(first, second):
        a = np.ascontiguousarray(first, dtype=np.float32).reshape(-1, 3)
        b = np.ascontiguousarray(second, dtype=np.float32).reshape(-1, 3)
        if len(a) != len(b):
            raise ValueError("the two ray arrays disagree in length")
        return a, b

    def trace_rays(self, origins, directions, device=0, keep_order=False, stats=False, force_regroup=False, posed=False):
        """bvh.intersect(&Ray::new(origin, direction)) per ray -> structured array (RAY_HIT_DTYPE) of n records
        {prim, t, p_hit, normal}; prim == NO_HIT is a miss.  Directions may have any length.  keep_order traces in the
        given order (no regrouping pass); the results are the same bytes either way."""
        o, d = self._ray_arrays(origins, directions)
        out = np.zeros(len(o), RAY_HIT_DTYPE)
        st = Stats()
        fn = _lib.rtx_trace_rays_posed if posed else _lib.rtx_trace_rays      # posed: against the device's pose (pose())
        _check(fn(self._h, device, len(o), _fp(o), _fp(d), self._ray_flags(keep_order, force_regroup),
                  out.ctypes.data_as(C.POINTER(RayHit)), C.byref(st) if stats else None), "rtx_trace_rays")
        return (out, st.asdict()) if stats else out

    def occluded_rays(self, origins, targets, device=0, keep_order=False, stats=False, force_regroup=False, posed=False):
        """The decision of main.rs:201-231 per (origin, target) pair -> uint8 [n], 1 = occluded, 0 = lit."""
        o, t = self._ray_arrays(origins, targets)
        out = np.zeros(len(o), np.uint8)
        st = Stats()
        fn = _lib.rtx_occluded_rays_posed if posed else _lib.rtx_occluded_rays
        _check(fn(self._h, device, len(o), _fp(o), _fp(t), self._ray_flags(keep_order, force_regroup),
                  out.ctypes.data_as(u8p), C.byref(st) if stats else None), "rtx_occluded_rays")
        return (out, st.asdict()) if stats else out

    def trace_rays_device(self, device, n_rays, d_origins_ptr, d_directions_ptr, d_hits_ptr, stream=None,
                          keep_order=False, force_regroup=False, posed=False):
        """Asynchronous closest-hit launch on device buffers the caller owns (n x 3 float32 twice, n x 32 bytes out)."""
        fn = _lib.rtx_trace_rays_posed_device if posed else _lib.rtx_trace_rays_device
        _check(fn(self._h, device, n_rays, C.c_void_p(d_origins_ptr), C.c_void_p(d_directions_ptr),
                  self._ray_flags(keep_order, force_regroup), C.c_void_p(d_hits_ptr),
                  C.c_void_p(stream) if stream else None), "rtx_trace_rays_device")

    def occluded_rays_device(self, device, n_rays, d_origins_ptr, d_targets_ptr, d_occluded_ptr, stream=None,
                             keep_order=False, force_regroup=False, posed=False):
        """Asynchronous occlusion launch on device buffers the caller owns (n x 3 float32 twice, n bytes out)."""
        fn = _lib.rtx_occluded_rays_posed_device if posed else _lib.rtx_occluded_rays_device
        _check(fn(self._h, device, n_rays, C.c_void_p(d_origins_ptr), C.c_void_p(d_targets_ptr),
                  self._ray_flags(keep_order, force_regroup), C.c_void_p(d_occluded_ptr),
                  C.c_void_p(stream) if stream else None), "rtx_occluded_rays_device")

    # -- shading rays the caller supplies (GPU only)
    @staticmethod
    def _lit_or_posed(stem, form, head, tail, light, posed):
        """Calls stem + form (form: "" or "_device"), its _lit twin under a light, or its _posed twin (whose light is
        optional: None is the scene's), with the light between head and tail."""
        if posed:
            name, mid = stem + "_posed" + form, (C.byref(light) if light is not None else None,)
        elif light is None:
            name, mid = stem + form, ()
        else:
            name, mid = stem + "_lit" + form, (C.byref(light),)
        _check(getattr(_lib, name)(*head, *mid, *tail), name)

    def shade_rays(self, origins, directions, device=0, keep_order=False, stats=False, force_regroup=False,
                   want_hits=False, light=None, posed=False):
        """render_pixel's body (main.rs:182-239) per pixel of nb_ray consecutive rays -> structured array
        (PIXEL_SHADE_DTYPE) of n / nb_ray records {linear, rgb8, hits}.  want_hits adds the rays' closest hits
        (RAY_HIT_DTYPE, n records, what trace_rays returns); stats adds the statistics, last.  Directions may have any
        length; keep_order shades in the given order (no regrouping pass): the same bytes either way.  light (an RtxLight:
        make_light, light()) shades under that light and sample count instead of the scene's (rtx_shade_rays_lit)."""
        o, d = self._ray_arrays(origins, directions)
        if len(o) % self.nb_ray:
            raise ValueError("a pixel is nb_ray = %d consecutive rays" % self.nb_ray)
        n = len(o) // self.nb_ray
        out = np.zeros(n, PIXEL_SHADE_DTYPE)
        hits = np.zeros(len(o), RAY_HIT_DTYPE) if want_hits else None
        st = Stats()
        tail = (out.ctypes.data_as(C.POINTER(PixelShade)), hits.ctypes.data_as(C.POINTER(RayHit)) if want_hits else None,
                C.byref(st) if stats else None)
        head = (self._h, device, n, _fp(o), _fp(d), self._ray_flags(keep_order, force_regroup))
        self._lit_or_posed("rtx_shade_rays", "", head, tail, light, posed)
        res = (out,) + ((hits,) if want_hits else ()) + ((st.asdict(),) if stats else ())
        return res if len(res) > 1 else out

    def shade_rays_device(self, device, n_pixels, d_origins_ptr, d_directions_ptr, d_shade_ptr, d_hits_ptr=None,
                          stream=None, keep_order=False, force_regroup=False, light=None, posed=False):
        """Asynchronous shading launch on device buffers the caller owns (n_pixels * nb_ray x 3 float32 twice,
        n_pixels x 16 bytes out, optionally n_pixels * nb_ray x 32 bytes of hit records)."""
        head = (self._h, device, n_pixels, C.c_void_p(d_origins_ptr), C.c_void_p(d_directions_ptr),
                self._ray_flags(keep_order, force_regroup))
        tail = (C.c_void_p(d_shade_ptr), C.c_void_p(d_hits_ptr) if d_hits_ptr else None, C.c_void_p(stream) if stream else None)
        self._lit_or_posed("rtx_shade_rays", "_device", head, tail, light, posed)

    # -- any pinhole view of the uploaded scene (GPU only)
    @staticmethod
    def view(width, height, eye, look_at, up=DEFAULT_UP, distance=DEFAULT_DISTANCE, rect=None):
        """An RtxView: a width x height frame seen through Camera::new(eye, look_at, up) at `distance` (camera_new);
        rect = (x0, y0, nx, ny) picks the pixels to render, default the whole frame."""
        u, v, w = camera_new(eye, look_at, up)
        x0, y0, nx, ny = (0, 0, width, height) if rect is None else rect
        out = RtxView(width=int(width), height=int(height), distance=float(distance), x0=int(x0), y0=int(y0), nx=int(nx), ny=int(ny))
        out.eye[:], out.u[:], out.v[:], out.w[:] = _f3(eye).tolist(), u.tolist(), v.tolist(), w.tolist()
        return out

    def own_view(self):
        """The scene's own camera and whole frame as an RtxView (rtx_scene_view)."""
        out = RtxView()
        _check(_lib.rtx_scene_view(self._h, C.byref(out)), "rtx_scene_view")
        return out

    def render_view(self, view, device=0, stats=False, want_shade=False, want_hits=False, light=None, posed=False):
        """render_pixel for every pixel of the view's rectangle -> uint8 [ny, nx, 3]; want_shade adds the pixels' records
        (PIXEL_SHADE_DTYPE [ny, nx]: what shade_rays returns for the view's rays), want_hits the rays' closest hits
        (RAY_HIT_DTYPE [ny, nx, nb_ray]: trace_rays'), stats the statistics, last.  light (an RtxLight: make_light, light())
        renders under that light and sample count instead of the scene's (rtx_render_view_lit)."""
        out = np.zeros((view.ny, view.nx, 3), np.uint8)
        shade = np.zeros((view.ny, view.nx), PIXEL_SHADE_DTYPE) if want_shade else None
        hits = np.zeros((view.ny, view.nx, self.nb_ray), RAY_HIT_DTYPE) if want_hits else None
        st = Stats()
        tail = (out.ctypes.data, shade.ctypes.data_as(C.POINTER(PixelShade)) if want_shade else None,
                hits.ctypes.data_as(C.POINTER(RayHit)) if want_hits else None, C.byref(st) if stats else None)
        self._lit_or_posed("rtx_render_view", "", (self._h, device, C.byref(view)), tail, light, posed)
        res = (out,) + ((shade,) if want_shade else ()) + ((hits,) if want_hits else ()) + ((st.asdict(),) if stats else ())
        return res if len(res) > 1 else out

    def render_view_device(self, device, view, d_rgb_ptr=None, d_shade_ptr=None, d_hits_ptr=None, stream=None, light=None,
                           posed=False):
        """Asynchronous view launch into device buffers the caller owns, each optional: ny*nx*3 bytes, ny*nx x 16 bytes,
        ny*nx*nb_ray x 32 bytes."""
        tail = (C.c_void_p(d_rgb_ptr) if d_rgb_ptr else None, C.c_void_p(d_shade_ptr) if d_shade_ptr else None,
                C.c_void_p(d_hits_ptr) if d_hits_ptr else None, C.c_void_p(stream) if stream else None)
        self._lit_or_posed("rtx_render_view", "_device", (self._h, device, C.byref(view)), tail, light, posed)

    # -- posing the scene's triangles (GPU only, posed_records and pose_bound aside): the posed= keyword of trace_rays*,
    #    occluded_rays*, shade_rays* and render_view* then works on the device's pose
    def pose_bound(self):
        """The largest coordinate magnitude a pose may hold (rtx_scene_pose_bound)."""
        out = C.c_float(0.0)
        _check(_lib.rtx_scene_pose_bound(self._h, C.byref(out)), "rtx_scene_pose_bound")
        return np.float32(out.value)

    def _pose_arrays(self, v0v1v2, tie_rank):
        v = np.ascontiguousarray(v0v1v2, dtype=np.float32).reshape(-1, 9)
        if len(v) != len(self.tris):
            raise ValueError("a pose has one entry per triangle of the scene")
        rank = None if tie_rank is None else np.ascontiguousarray(tie_rank, dtype=np.uint32).reshape(-1)
        if rank is not None and len(rank) != self.n_prims:
            raise ValueError("tie_rank must have one entry per primitive")
        return v, rank

    def _pose(self, name, device, head, rebuilt=None, reference_tree=None, stats=False, stream=None):
        """One pose entry point: `head` (the arrays, or the struct), the flag word where the entry point has one (rebuilt is
        not None), then reference_tree and stats (a host form: reference_tree is not None) or the stream -> the stats dict
        or None"""
        st = Stats()
        args = list(head) + ([POSE_REBUILT if rebuilt else 0] if rebuilt is not None else [])
        if reference_tree is not None:
            args += [int(reference_tree), C.byref(st) if stats else None]
        else:
            args.append(C.c_void_p(stream) if stream else None)
        _check(getattr(_lib, name)(self._h, device, *args), name)
        return st.asdict() if stats else None

    def pose(self, v0v1v2, device=0, tie_rank=None, reference_tree=REFTREE_NEVER, stats=False):
        """Moves the scene's triangles on `device` to v0v1v2 (float32 [n_tris, 9], Vec order, spheres skipped): one pose per
        scene and device, replaced by the next (rtx_scene_pose).  stats: kernel_ms is the pose kernels' time."""
        v, rank = self._pose_arrays(v0v1v2, tie_rank)
        return self._pose("rtx_scene_pose", device, (_fp(v), _up(rank)), None, reference_tree, stats)

    def pose_device(self, device, d_v0v1v2_ptr, d_tie_rank_ptr=None, stream=None):
        """Asynchronous pose from device arrays the caller owns (n_tris x 9 float32; n_prims uint32 or None)."""
        self._pose("rtx_scene_pose_device", device, (C.c_void_p(d_v0v1v2_ptr), C.c_void_p(d_tie_rank_ptr) if d_tie_rank_ptr else None),
                   stream=stream)

    def _pose_outputs(self, rebuilt=False):
        """-> zeroed (tris, shade, nodes), a rebuilt pose's: (perm, tris, shade, nodes)"""
        t, s = np.zeros((self.n_prims, 16), np.uint32), np.zeros((self.n_prims, 8), np.uint32)
        if rebuilt:
            return np.zeros(self.n_prims - self.info()["n_global"], np.uint32), t, s, np.zeros((self.rebuilt_counts(), 8), np.uint32)
        return t, s, np.zeros((self.info()["n_nodes"], 8), np.uint32)

    def _prim_outputs(self):
        """-> zeroed (v0v1v2 [n_tris, 9], spheres [n_spheres, 4])"""
        return np.zeros((len(self.tris), 9), np.float32), np.zeros((len(self.spheres), 4), np.float32)

    def posed_records(self, v0v1v2, tie_rank=None):
        """Host only: the words the pose kernels make -> (tris uint32 [n_prims, 16] in leaf order, shade uint32 [n_prims, 8]
        in Vec order, nodes uint32 [n_nodes, 8] in nodes()' word order with the planes moved by cull_delta)."""
        v, rank = self._pose_arrays(v0v1v2, tie_rank)
        t, s, n = self._pose_outputs()
        _check(_lib.rtx_scene_posed_records(self._h, _fp(v), _up(rank), _up(t), _up(s), _up(n)), "rtx_scene_posed_records")
        return t, s, n

    def debug_pose(self, device=0):
        """Diagnostics: the pose `device` holds, copied back, in posed_records' layout."""
        t, s, n = self._pose_outputs()
        _check(_lib.rtx_debug_pose(self._h, device, _up(t), _up(s), _up(n)), "rtx_debug_pose")
        return t, s, n

    # -- another light for views and shaded rays: the light= keyword of render_view* and shade_rays*
    @staticmethod
    def make_light(light_tri, nb_light_sample=0):
        """An RtxLight: the nine floats of Light.primitives[0] (v0, v1, v2) and the sample count, 0 = the scene's."""
        lt = np.asarray(light_tri, dtype=np.float32).reshape(9)
        out = RtxLight(nb_light_sample=int(nb_light_sample))
        out.v0[:], out.v1[:], out.v2[:] = lt[0:3].tolist(), lt[3:6].tolist(), lt[6:9].tolist()
        return out

    def light(self):
        """The light and sample count the scene was created with, as an RtxLight (rtx_scene_light)."""
        out = RtxLight()
        _check(_lib.rtx_scene_light(self._h, C.byref(out)), "rtx_scene_light")
        return out

    def light_points_for(self, light):
        """Host only: float32 [nb_ray * n, 3], the points of `light` on this scene (n: its count, or the scene's for 0)."""
        n = _lib.rtx_scene_light_points_for(self._h, C.byref(light), None)
        if n < 0:
            raise RtxError(n, "rtx_scene_light_points_for")
        out = np.zeros((n, 3), np.float32)
        if n and _lib.rtx_scene_light_points_for(self._h, C.byref(light), _fp(out)) != n:
            raise RtxError(ERR_INTERNAL, "rtx_scene_light_points_for")
        return out

    def debug_light_points(self, light, device=0):
        """Diagnostics: the same points as the light kernel makes them on `device`, copied back."""
        n = _lib.rtx_scene_light_points_for(self._h, C.byref(light), None)
        if n < 0:
            raise RtxError(n, "rtx_scene_light_points_for")
        out = np.zeros((max(n, 1), 3), np.float32)
        _check(_lib.rtx_debug_light_points(self._h, device, C.byref(light), _fp(out)), "rtx_debug_light_points")
        return out[:n]

    def light_walk_for(self, light):
        """Host only: what the walk kernels make for `light` on this scene -> (order uint32 [nb_ray * n] in light_order()'s
        form, boxes float32 [nb_ray, 6], shaft_delta float32)."""
        n = _lib.rtx_scene_light_walk_for(self._h, C.byref(light), None, None, None)
        if n < 0:
            raise RtxError(n, "rtx_scene_light_walk_for")
        order = np.zeros(max(n, 1), np.uint32)
        boxes = np.zeros((self.nb_ray, 6), np.float32)
        delta = C.c_float(0.0)
        if _lib.rtx_scene_light_walk_for(self._h, C.byref(light), order.ctypes.data_as(u32p), _fp(boxes), C.byref(delta)) != n:
            raise RtxError(ERR_INTERNAL, "rtx_scene_light_walk_for")
        return order[:n], boxes, np.float32(delta.value)

    def light_walk_seeded(self, seed, n_pairs, light=None):
        """Host only: light_walk_for's outputs on a scene reseeded with (seed, n_pairs), this scene unchanged — what a frame of
        render_view_mean(rows=True) walks (rtx_scene_light_walk_seeded).  light: None, the scene's."""
        lp = C.byref(light) if light is not None else None
        n = _lib.rtx_scene_light_walk_seeded(self._h, lp, int(seed) & 0xFFFFFFFFFFFFFFFF, int(n_pairs), None, None, None)
        if n < 0:
            raise RtxError(n, "rtx_scene_light_walk_seeded")
        order = np.zeros(max(n, 1), np.uint32)
        boxes = np.zeros((self.nb_ray, 6), np.float32)
        delta = C.c_float(0.0)
        if _lib.rtx_scene_light_walk_seeded(self._h, lp, int(seed) & 0xFFFFFFFFFFFFFFFF, int(n_pairs), order.ctypes.data_as(u32p),
                                            _fp(boxes), C.byref(delta)) != n:
            raise RtxError(ERR_INTERNAL, "rtx_scene_light_walk_seeded")
        return order[:n], boxes, np.float32(delta.value)

    def debug_light_walk(self, light, device=0):
        """Diagnostics: the tour records (uint32 [nb_ray * n, 4]: x, y, z bits and the index within the batch) and the boxes
        (float32 [nb_ray, 6]) as the light kernels make them on `device`, copied back."""
        n = _lib.rtx_scene_light_points_for(self._h, C.byref(light), None)
        if n < 0:
            raise RtxError(n, "rtx_scene_light_points_for")
        tour = np.zeros((max(n, 1), 4), np.uint32)
        boxes = np.zeros((self.nb_ray, 6), np.float32)
        _check(_lib.rtx_debug_light_walk(self._h, device, C.byref(light), tour.ctypes.data_as(f32p), _fp(boxes)),
               "rtx_debug_light_walk")
        return tour[:n], boxes

    # -- any view through the render pipeline (GPU only); light=: under another light (rtx_render_view_rows_lit)
    def render_view_rows(self, view, device=0, stats=False, light=None, posed=False):
        """Rows [y0, y0 + ny) of the view's frame through the render pipeline, full width (x0 = 0, nx = width)
        -> uint8 [ny, width, 3]: render_view's bytes at the pipeline's speed.  An eye beyond the scene's largest
        coordinate raises RtxError(ERR_UNSUPPORTED): render_view serves it.  posed: the device's pose (pose()) in place of
        the uploaded triangles (rtx_render_view_rows_posed)."""
        out = np.zeros((view.ny, view.width, 3), np.uint8)
        st = Stats()
        self._lit_or_posed("rtx_render_view_rows", "", (self._h, device, C.byref(view)),
                           (out.ctypes.data, C.byref(st) if stats else None), light, posed)
        return (out, st.asdict()) if stats else out

    def render_view_rows_device(self, device, view, d_rgb_ptr, d_bytes, stream=None, d_counters_ptr=None, light=None, posed=False):
        """Asynchronous pipeline launch of the view's rows into a device buffer the caller owns (ny*width*3 bytes)."""
        tail = (C.c_void_p(d_rgb_ptr), d_bytes, C.c_void_p(stream) if stream else None,
                C.c_void_p(d_counters_ptr) if d_counters_ptr else None)
        self._lit_or_posed("rtx_render_view_rows", "_device", (self._h, device, C.byref(view)), tail, light, posed)

    # -- the pipeline's linear output: the RtxPixelShade records of render_view, at the pipeline's speed
    def render_view_rows_shade(self, view, device=0, stats=False, light=None, posed=False):
        """Rows [y0, y0 + ny) of the view's frame through the render pipeline as records -> PIXEL_SHADE_DTYPE [ny, width]:
        render_view's `shade` (linear sums bit for bit, bytes, hit counts), light= and posed= as render_view_rows
        (rtx_render_view_rows_shade)."""
        out = np.zeros((view.ny, view.width), PIXEL_SHADE_DTYPE)
        st = Stats()
        _check(_lib.rtx_render_view_rows_shade(self._h, device, C.byref(view), C.byref(light) if light is not None else None,
                                               ROWS_POSED if posed else 0, out.ctypes.data_as(C.POINTER(PixelShade)),
                                               C.byref(st) if stats else None), "rtx_render_view_rows_shade")
        return (out, st.asdict()) if stats else out

    def render_view_rows_shade_device(self, device, view, d_shade_ptr, d_bytes, stream=None, d_counters_ptr=None, light=None,
                                      posed=False):
        """Asynchronous pipeline launch of the view's rows as records into a device buffer the caller owns (ny*width*16
        bytes, 16-byte aligned)."""
        _check(_lib.rtx_render_view_rows_shade_device(self._h, device, C.byref(view), C.byref(light) if light is not None else None,
                                                      ROWS_POSED if posed else 0, C.c_void_p(d_shade_ptr), d_bytes,
                                                      C.c_void_p(stream) if stream else None,
                                                      C.c_void_p(d_counters_ptr) if d_counters_ptr else None),
               "rtx_render_view_rows_shade_device")

    def aimed_nodes(self, eye):
        """Host only: records [n_nodes, 8] of the stream the primary rays of a view with this eye walk (planes moved by
        cull_delta, the child nearer the eye first), NodeRec word order as nodes()."""
        nd = np.zeros((self.info()["n_nodes"], 8), np.uint32)
        _check(_lib.rtx_scene_aimed_nodes(self._h, _fp(_f3(eye)), nd.ctypes.data_as(u32p)), "rtx_scene_aimed_nodes")
        return nd

    def debug_aimed_nodes(self, eye, device=0):
        """Diagnostics: the same stream as the aim kernels make it on `device`, copied back, same word order."""
        nd = np.zeros((self.info()["n_nodes"], 8), np.uint32)
        _check(_lib.rtx_debug_aimed_nodes(self._h, device, _fp(_f3(eye)), nd.ctypes.data_as(u32p)), "rtx_debug_aimed_nodes")
        return nd

    # -- the pose through the render pipeline: the posed= keyword of render_view_rows*; what it reads beside the pose
    def _pipeline_outputs(self):
        i = self.info()
        return np.zeros((i["n_global"], 16), np.uint32), np.zeros((i["n_nodes"], 8), np.uint32)

    def posed_pipeline_records(self, v0v1v2, eye=None):
        """Host only: the words a pose makes for the pipeline -> (planes uint32 [n_global, 16], aimed uint32 [n_nodes, 8] in
        aimed_nodes()' word order, or None without an eye)."""
        v, _ = self._pose_arrays(v0v1v2, None)
        planes, aimed = self._pipeline_outputs()
        _check(_lib.rtx_scene_posed_pipeline_records(self._h, _fp(v), _fp(_f3(eye)) if eye is not None else None,
                                                     planes.ctypes.data_as(u32p),
                                                     aimed.ctypes.data_as(u32p) if eye is not None else None),
               "rtx_scene_posed_pipeline_records")
        return planes, (aimed if eye is not None else None)

    def debug_pose_pipeline(self, eye=None, device=0):
        """Diagnostics: the plane records of the pose `device` holds and the aim kernels run over it for `eye`, copied back,
        in posed_pipeline_records' layout."""
        planes, aimed = self._pipeline_outputs()
        _check(_lib.rtx_debug_pose_pipeline(self._h, device, _fp(_f3(eye)) if eye is not None else None,
                                            planes.ctypes.data_as(u32p), aimed.ctypes.data_as(u32p) if eye is not None else None),
               "rtx_debug_pose_pipeline")
        return planes, (aimed if eye is not None else None)

    # -- a pose whose tree is rebuilt on the device: every posed= call then runs over it unchanged
    def pose_rebuilt(self, v0v1v2, device=0, tie_rank=None, reference_tree=REFTREE_NEVER, stats=False):
        """pose() with the tree rebuilt on the device: the tree proper's records sorted by Morton key, a balanced tree over
        the sorted runs, boxes by the refit kernels (rtx_scene_pose_rebuilt).  stats: kernel_ms is the kernels' time."""
        v, rank = self._pose_arrays(v0v1v2, tie_rank)
        return self._pose("rtx_scene_pose_rebuilt", device, (_fp(v), _up(rank)), None, reference_tree, stats)

    def pose_rebuilt_device(self, device, d_v0v1v2_ptr, d_tie_rank_ptr=None, stream=None):
        """Asynchronous rebuilt pose from device arrays the caller owns (n_tris x 9 float32; n_prims uint32 or None)."""
        self._pose("rtx_scene_pose_rebuilt_device", device,
                   (C.c_void_p(d_v0v1v2_ptr), C.c_void_p(d_tie_rank_ptr) if d_tie_rank_ptr else None), stream=stream)

    def rebuilt_counts(self):
        """Node records of the rebuilt stream (rtx_scene_rebuilt_counts)."""
        out = C.c_uint32(0)
        _check(_lib.rtx_scene_rebuilt_counts(self._h, C.byref(out)), "rtx_scene_rebuilt_counts")
        return int(out.value)

    def rebuilt_records(self, v0v1v2, tie_rank=None):
        """Host only: the words a rebuilt pose makes -> (keys uint64 [n_tree], perm uint32 [n_tree] — positions of the
        uploaded primitive array in sorted order —, tris uint32 [n_prims, 16] in sorted order, shade uint32 [n_prims, 8] in
        Vec order, nodes uint32 [rebuilt_counts(), 8] with the planes moved by cull_delta)."""
        v, rank = self._pose_arrays(v0v1v2, tie_rank)
        perm, t, s, n = self._pose_outputs(rebuilt=True)
        keys = np.zeros(len(perm), np.uint64)
        _check(_lib.rtx_scene_rebuilt_records(self._h, _fp(v), _up(rank), keys.ctypes.data_as(C.POINTER(C.c_uint64)), _up(perm),
                                              _up(t), _up(s), _up(n)), "rtx_scene_rebuilt_records")
        return keys, perm, t, s, n

    def rebuilt_aimed(self, v0v1v2, eye):
        """Host only: the aim kernels' output over the rebuilt pose for `eye` -> uint32 [rebuilt_counts(), 8]."""
        v, _ = self._pose_arrays(v0v1v2, None)
        aimed = np.zeros((self.rebuilt_counts(), 8), np.uint32)
        _check(_lib.rtx_scene_rebuilt_aimed(self._h, _fp(v), _fp(_f3(eye)), _up(aimed)), "rtx_scene_rebuilt_aimed")
        return aimed

    def debug_pose_rebuilt(self, eye=None, device=0):
        """Diagnostics: the rebuilt pose `device` holds, copied back -> (perm, tris, shade, nodes, aimed or None without an
        eye), in rebuilt_records' layout; aimed: the aim kernels run over it for `eye`."""
        perm, t, s, n = self._pose_outputs(rebuilt=True)
        aimed = np.zeros_like(n) if eye is not None else None
        _check(_lib.rtx_debug_pose_rebuilt(self._h, device, _fp(_f3(eye)) if eye is not None else None, _up(perm), _up(t), _up(s),
                                           _up(n), _up(aimed)), "rtx_debug_pose_rebuilt")
        return perm, t, s, n, aimed

    # -- a pose that states every field of a primitive: spheres move, colours change.  None = as uploaded
    def _prims_struct(self, v0v1v2, spheres, rgb, sphere_rgb, tie_rank):
        """-> (RtxPosePrims of host pointers, the arrays they point into)"""
        def shaped(a, rows, cols, what):
            if a is None:
                return None
            a = np.ascontiguousarray(a, dtype=np.float32).reshape(-1, cols)
            if len(a) != rows:
                raise ValueError("a pose has one entry per %s of the scene" % what)
            return a
        v, rank = self._pose_arrays(self.tris if v0v1v2 is None else v0v1v2, tie_rank)
        keep = [v, shaped(spheres, len(self.spheres), 4, "sphere"), shaped(rgb, len(self.tris), 3, "triangle"),
                shaped(sphere_rgb, len(self.spheres), 3, "sphere"), rank]
        return RtxPosePrims(*[a.ctypes.data if a is not None and a.size else None for a in keep]), keep

    def pose_prims(self, v0v1v2=None, spheres=None, rgb=None, sphere_rgb=None, device=0, tie_rank=None,
                   reference_tree=REFTREE_NEVER, rebuilt=False, stats=False):
        """pose() / pose_rebuilt() with the spheres (float32 [n_spheres, 4]: origin, radius) and the colours of both arms
        (float32 [n_tris, 3], [n_spheres, 3]) stated too; None: as uploaded (v0v1v2: the scene's own vertices)
        (rtx_scene_pose_prims).  stats: kernel_ms is the kernels' time, the overlay kernel's included."""
        prims, keep = self._prims_struct(v0v1v2, spheres, rgb, sphere_rgb, tie_rank)
        return self._pose("rtx_scene_pose_prims", device, (C.byref(prims),), rebuilt, reference_tree, stats)

    def pose_prims_device(self, device, d_v0v1v2_ptr, d_spheres_ptr=None, d_rgb_ptr=None, d_sphere_rgb_ptr=None,
                          d_tie_rank_ptr=None, rebuilt=False, stream=None):
        """Asynchronous pose of every field from device arrays the caller owns (None or 0: as uploaded)."""
        prims = RtxPosePrims(*[p if p else None for p in (d_v0v1v2_ptr, d_spheres_ptr, d_rgb_ptr, d_sphere_rgb_ptr, d_tie_rank_ptr)])
        self._pose("rtx_scene_pose_prims_device", device, (C.byref(prims),), rebuilt, stream=stream)

    def pose_prims_records(self, v0v1v2=None, spheres=None, rgb=None, sphere_rgb=None, tie_rank=None, rebuilt=False):
        """Host only: the words such a pose makes -> posed_records' (tris, shade, nodes), or with rebuilt=True
        rebuilt_records' (keys, perm, tris, shade, nodes)."""
        prims, keep = self._prims_struct(v0v1v2, spheres, rgb, sphere_rgb, tie_rank)
        perm, t, s, n = self._pose_outputs(rebuilt=True) if rebuilt else (None,) + self._pose_outputs()
        keys = np.zeros(len(perm), np.uint64) if rebuilt else None
        _check(_lib.rtx_scene_pose_prims_records(self._h, C.byref(prims), POSE_REBUILT if rebuilt else 0,
                                                 keys.ctypes.data_as(C.POINTER(C.c_uint64)) if rebuilt else None, _up(perm), _up(t),
                                                 _up(s), _up(n)), "rtx_scene_pose_prims_records")
        return (keys, perm, t, s, n) if rebuilt else (t, s, n)

    def pose_prims_aimed(self, eye, v0v1v2=None, spheres=None, rgb=None, sphere_rgb=None, rebuilt=False):
        """Host only: the aim kernels' output over such a pose for `eye` -> uint32 [n_nodes or rebuilt_counts(), 8]."""
        prims, keep = self._prims_struct(v0v1v2, spheres, rgb, sphere_rgb, None)
        aimed = np.zeros((self.rebuilt_counts() if rebuilt else self.info()["n_nodes"], 8), np.uint32)
        _check(_lib.rtx_scene_pose_prims_aimed(self._h, C.byref(prims), POSE_REBUILT if rebuilt else 0, _fp(_f3(eye)), _up(aimed)),
               "rtx_scene_pose_prims_aimed")
        return aimed

    # -- a pose the device makes from the scene's geometry as created and a set of affine moves
    def _moves_struct(self, moves, group, radius_scale, rgb=None, sphere_rgb=None, tie_rank=None):
        """-> (RtxPoseMoves of host pointers, the arrays they point into)"""
        m = np.ascontiguousarray(moves, dtype=np.float32).reshape(-1, 12)
        g = None if group is None else np.ascontiguousarray(group, dtype=np.uint32).reshape(-1)
        if g is not None and len(g) != self.n_prims:
            raise ValueError("group has one entry per primitive of the scene")
        r = None if radius_scale is None else np.ascontiguousarray(radius_scale, dtype=np.float32).reshape(-1)
        if r is not None and len(r) != len(m):
            raise ValueError("radius_scale has one entry per move")
        prims, keep = self._prims_struct(None, None, rgb, sphere_rgb, tie_rank)
        keep = [m, g, r] + keep
        addr = lambda a: a.ctypes.data if a is not None and a.size else None
        return RtxPoseMoves(len(m), addr(m), addr(g), addr(r), prims.rgb, prims.sphere_rgb, prims.tie_rank), keep

    def pose_moved(self, moves, group=None, radius_scale=None, rgb=None, sphere_rgb=None, device=0, tie_rank=None,
                   reference_tree=REFTREE_NEVER, rebuilt=False, stats=False):
        """pose_prims() with the vertices and the spheres made ON THE DEVICE: moves float32 [n_moves, 12] (3 x 4 maps, row
        major), group uint32 [n_prims] (the move each Vec position follows, MOVE_NONE: none; None: all follow move 0),
        radius_scale float32 [n_moves] or None (rtx_scene_pose_moved).  stats: kernel_ms includes the move kernel."""
        mv, keep = self._moves_struct(moves, group, radius_scale, rgb, sphere_rgb, tie_rank)
        return self._pose("rtx_scene_pose_moved", device, (C.byref(mv),), rebuilt, reference_tree, stats)

    def pose_moved_device(self, device, n_moves, d_moves_ptr, d_group_ptr=None, d_radius_scale_ptr=None, d_rgb_ptr=None,
                          d_sphere_rgb_ptr=None, d_tie_rank_ptr=None, rebuilt=False, stream=None):
        """Asynchronous moved pose from device arrays the caller owns (None or 0: no such array)."""
        mv = RtxPoseMoves(int(n_moves), *[p if p else None for p in (d_moves_ptr, d_group_ptr, d_radius_scale_ptr, d_rgb_ptr,
                                                                     d_sphere_rgb_ptr, d_tie_rank_ptr)])
        self._pose("rtx_scene_pose_moved_device", device, (C.byref(mv),), rebuilt, stream=stream)

    def moved_prims(self, moves, group=None, radius_scale=None):
        """Host only: the arrays such a pose makes -> (v0v1v2 float32 [n_tris, 9], spheres float32 [n_spheres, 4])
        (rtx_scene_moved_prims)."""
        mv, keep = self._moves_struct(moves, group, radius_scale)
        v, sph = self._prim_outputs()
        _check(_lib.rtx_scene_moved_prims(self._h, C.byref(mv), _fp(v), _fp(sph)), "rtx_scene_moved_prims")
        return v, sph

    def debug_moved_prims(self, device=0):
        """Diagnostic: the arrays the move kernel last wrote on `device`, in moved_prims' form (rtx_debug_moved_prims)."""
        v, sph = self._prim_outputs()
        _check(_lib.rtx_debug_moved_prims(self._h, device, _fp(v), _fp(sph)), "rtx_debug_moved_prims")
        return v, sph

    # -- a skin bound once, and poses that blend up to four moves per triangle corner on the device
    def skin(self, bones=None, weights=None, sphere_bone=None):
        """Binds a skin (rtx_scene_skin; the arrays are copied): bones uint32 [n_tris, 3, 4] and weights float32
        [n_tris, 3, 4] per corner, sphere_bone uint32 [n_spheres] or None (every sphere MOVE_NONE).  skin() with no
        argument unbinds.  Not re-entrant per scene."""
        if bones is None and weights is None and sphere_bone is None:
            _check(_lib.rtx_scene_skin(self._h, None), "rtx_scene_skin")
            return
        n_tris, n_spheres = len(self.tris), len(self.spheres)
        b = np.ascontiguousarray(bones if bones is not None else np.zeros((0, 3, 4)), dtype=np.uint32).reshape(-1)
        w = np.ascontiguousarray(weights if weights is not None else np.zeros((0, 3, 4)), dtype=np.float32).reshape(-1)
        if len(b) != 12 * n_tris or len(w) != 12 * n_tris:
            raise ValueError("bones and weights have 3 x 4 entries per triangle of the scene")
        s = None if sphere_bone is None else np.ascontiguousarray(sphere_bone, dtype=np.uint32).reshape(-1)
        if s is not None and len(s) != n_spheres:
            raise ValueError("sphere_bone has one entry per sphere of the scene")
        addr = lambda a: a.ctypes.data if a is not None and a.size else None
        _check(_lib.rtx_scene_skin(self._h, C.byref(RtxSkin(addr(b), addr(w), addr(s)))), "rtx_scene_skin")

    def skin_bound(self):
        """-> (bound, the largest bone other than MOVE_NONE) (rtx_scene_skin_bound)"""
        top = C.c_uint32(0)
        rc = _lib.rtx_scene_skin_bound(self._h, C.byref(top))
        if rc < 0:
            _check(rc, "rtx_scene_skin_bound")
        return bool(rc), int(top.value)

    def pose_skinned(self, moves, radius_scale=None, rgb=None, sphere_rgb=None, device=0, tie_rank=None,
                     reference_tree=REFTREE_NEVER, rebuilt=False, stats=False):
        """pose_moved() with the bound skin naming the moves: every triangle corner blends up to four of them
        (rtx_scene_pose_skinned).  stats: kernel_ms includes the skin kernel."""
        mv, keep = self._moves_struct(moves, None, radius_scale, rgb, sphere_rgb, tie_rank)
        return self._pose("rtx_scene_pose_skinned", device, (C.byref(mv),), rebuilt, reference_tree, stats)

    def pose_skinned_device(self, device, n_moves, d_moves_ptr, d_radius_scale_ptr=None, d_rgb_ptr=None, d_sphere_rgb_ptr=None,
                            d_tie_rank_ptr=None, rebuilt=False, stream=None):
        """Asynchronous skinned pose from device arrays the caller owns (None or 0: no such array)."""
        mv = RtxPoseMoves(int(n_moves), *[p if p else None for p in (d_moves_ptr, None, d_radius_scale_ptr, d_rgb_ptr,
                                                                     d_sphere_rgb_ptr, d_tie_rank_ptr)])
        self._pose("rtx_scene_pose_skinned_device", device, (C.byref(mv),), rebuilt, stream=stream)

    def skinned_prims(self, moves, radius_scale=None):
        """Host only: the arrays such a pose makes -> (v0v1v2 float32 [n_tris, 9], spheres float32 [n_spheres, 4])
        (rtx_scene_skinned_prims)."""
        mv, keep = self._moves_struct(moves, None, radius_scale)
        v, sph = self._prim_outputs()
        _check(_lib.rtx_scene_skinned_prims(self._h, C.byref(mv), _fp(v), _fp(sph)), "rtx_scene_skinned_prims")
        return v, sph

    # -- the sample table replaced: a caller's table, or a seeded one each device makes from the seed
    def resample(self, samples):
        """Replaces the scene's sample table by `samples` (float32 [n, 2], copied: rtx_scene_resample).  Host only; every
        device catches up in its next call.  Every later call answers as a scene created with this table would."""
        t = np.ascontiguousarray(samples, dtype=np.float32).reshape(-1, 2)
        _check(_lib.rtx_scene_resample(self._h, _fp(t), len(t)), "rtx_scene_resample")
        self.samples = t

    def reseed(self, seed=DEFAULT_SEED, n_pairs=NB_RAND_SAMPLE):
        """Replaces the scene's sample table by gen_samples(seed, n_pairs), which is never made on the host: each device
        makes its copy from the seed (rtx_scene_reseed).  self.samples becomes None: read it with samples_at()."""
        _check(_lib.rtx_scene_reseed(self._h, int(seed) & 0xFFFFFFFFFFFFFFFF, int(n_pairs)), "rtx_scene_reseed")
        self.samples = None

    def n_samples(self):
        """pairs of the scene's current table"""
        return self.info()["sample_bytes"] // 8

    def samples_at(self, first=0, count=None):
        """Host only: `count` pairs of the scene's current table from pair `first` -> float32 [count, 2]
        (rtx_scene_samples; default: to the end)"""
        count = self.n_samples() - first if count is None else count
        out = np.zeros((count, 2), np.float32)
        _check(_lib.rtx_scene_samples(self._h, int(first), int(count), _fp(out)), "rtx_scene_samples")
        return out

    def debug_samples(self, first=0, count=None, device=0):
        """The same range of the table `device` holds, after it caught up (rtx_debug_samples; blocks)"""
        count = self.n_samples() - first if count is None else count
        out = np.zeros((count, 2), np.float32)
        _check(_lib.rtx_debug_samples(self._h, device, int(first), int(count), _fp(out)), "rtx_debug_samples")
        return out

    # -- the mean of N frames, accumulated on the device: the scene is not changed
    @staticmethod
    def _seeds(seeds):
        return np.ascontiguousarray([int(x) & 0xFFFFFFFFFFFFFFFF for x in seeds], dtype=np.uint64)

    def _mean_call(self, name, device, view, light, flags, seeds, n_pairs, rule=None, tail=(), want=None):
        """One call of the mean family: the argument head all of them share (view, light, flags, seeds, n_frames, n_pairs;
        `rule`: the adaptive calls' RtxAdaptRule behind it), then `tail`, a device-resident call's pointers (None or 0:
        NULL), or with want = (shade, tiles, stats) a host call's outputs, made here and answered as (out, shade, tiles,
        stats) without the unwanted ones, `out` alone when nothing else is wanted."""
        sd = self._seeds(seeds)
        args = [self._h, device, C.byref(view), C.byref(light) if light is not None else None, flags, sd.ctypes.data_as(u64p),
                len(sd), int(n_pairs)]
        if rule is not None:
            args.append(C.byref(AdaptRule(int(rule[0]), float(rule[1]))))
        args += [C.c_void_p(p) if p else None for p in tail]
        if want is not None:
            want_shade, want_tiles, stats = want
            out = np.zeros((view.ny, view.nx, 3), np.uint8)
            shade = np.zeros((view.ny, view.nx), PIXEL_SHADE_DTYPE) if want_shade else None
            tiles = np.zeros(tile_grid(view.nx, view.ny)[::-1], TILE_STATE_DTYPE) if want_tiles else None
            st = Stats()
            args += [out.ctypes.data, shade.ctypes.data_as(C.POINTER(PixelShade)) if want_shade else None]
            if rule is not None:
                args.append(tiles.ctypes.data_as(C.POINTER(TileState)) if want_tiles else None)
            args.append(C.byref(st) if stats else None)
        _check(getattr(_lib, name)(*args), name)
        if want is None:
            return None
        res = tuple(x for x in (out, shade, tiles) if x is not None) + ((st.asdict(),) if stats else ())
        return res if len(res) > 1 else out

    def render_view_mean(self, view, seeds, n_pairs=NB_RAND_SAMPLE, device=0, light=None, posed=False, stats=False,
                         want_shade=False, rows=False):
        """The mean of len(seeds) frames of the view, frame k under the table gen_samples(seeds[k], n_pairs), summed in
        frame order and divided once (rtx_render_view_mean) -> uint8 [ny, nx, 3]; want_shade adds the records
        (PIXEL_SHADE_DTYPE [ny, nx]: the mean's linear colour, its bytes, in how many frames the pixel had a hit), stats
        the statistics summed over the frames, last.  light: an RtxLight, None the scene's; posed: the device's pose.
        rows: through the render pipeline (rtx_render_view_rows_mean: full width only, the same words)."""
        return self._mean_call("rtx_render_view_rows_mean" if rows else "rtx_render_view_mean", device, view, light,
                               MEAN_POSED if posed else 0, seeds, n_pairs, want=(want_shade, False, stats))

    def render_view_mean_device(self, device, view, seeds, n_pairs, d_accum_ptr, d_rgb_ptr=None, d_shade_ptr=None, stream=None,
                                light=None, posed=False, rows=False):
        """Asynchronous: the same chain on `stream` into device buffers the caller owns — ny*nx x 16 bytes of accumulator
        (16-byte aligned), optionally ny*nx*3 bytes (any alignment) and ny*nx x 16 bytes of records."""
        self._mean_call("rtx_render_view_rows_mean_device" if rows else "rtx_render_view_mean_device",      # (rows: through the pipeline)
                        device, view, light, MEAN_POSED if posed else 0, seeds, n_pairs, tail=(d_accum_ptr, d_rgb_ptr, d_shade_ptr, stream))

    def accum_add_device(self, device, n, d_shade_ptr, d_accum_ptr, first, stream=None):
        """Asynchronous: adds n RtxPixelShade records — of any call that writes them — into n accumulator records
        (rtx_accum_add_device); first: the accumulator is written, never read."""
        _check(_lib.rtx_accum_add_device(self._h, device, int(n), C.c_void_p(d_shade_ptr), C.c_void_p(d_accum_ptr), 1 if first else 0,
                                         C.c_void_p(stream) if stream else None), "rtx_accum_add_device")

    def accum_resolve_device(self, device, n, d_accum_ptr, n_frames, d_rgb_ptr=None, d_shade_ptr=None, stream=None):
        """Asynchronous: n accumulator records over n_frames frames into n*3 bytes (any alignment) and / or n records
        (rtx_accum_resolve_device), through the scene's gamma thresholds."""
        _check(_lib.rtx_accum_resolve_device(self._h, device, int(n), C.c_void_p(d_accum_ptr), int(n_frames),
                                             C.c_void_p(d_rgb_ptr) if d_rgb_ptr else None,
                                             C.c_void_p(d_shade_ptr) if d_shade_ptr else None,
                                             C.c_void_p(stream) if stream else None), "rtx_accum_resolve_device")

    # -- the adaptive mean of N frames: tiles stop once their noise estimate is met; the scene is not changed
    def render_view_adaptive(self, view, seeds, rule, n_pairs=NB_RAND_SAMPLE, device=0, light=None, posed=False, stats=False,
                             want_shade=False, want_tiles=False):
        """The mean of up to len(seeds) frames of the view (rtx_render_view_adaptive): an 8 x 8 tile of the rectangle stops
        receiving frames once it has rule[0] = min_frames of them and its noise estimate is <= rule[1] = max_variance
        -> uint8 [ny, nx, 3]; want_shade adds the records, want_tiles the tile states (TILE_STATE_DTYPE [tiles_y, tiles_x]:
        the frames each tile received and its estimate), stats the statistics summed over the rendered tile-frames, last."""
        return self._mean_call("rtx_render_view_adaptive", device, view, light, MEAN_POSED if posed else 0, seeds, n_pairs, rule=rule,
                               want=(want_shade, want_tiles, stats))

    def render_view_adaptive_device(self, device, view, seeds, rule, n_pairs, d_moments_ptr, d_tiles_ptr, d_rgb_ptr=None,
                                    d_shade_ptr=None, stream=None, light=None, posed=False, resume=False):
        """Asynchronous: the same chain on `stream` into device buffers the caller owns — ny*nx x 32 bytes of moments (16-byte
        aligned), tiles_y*tiles_x x 8 bytes of tile states (8-byte aligned), optionally ny*nx*3 bytes (any alignment) and
        ny*nx x 16 bytes of records.  resume (RTX_ADAPT_CONTINUE): the moments and the states are an earlier call's, the
        seeds the next frames'."""
        flags = (MEAN_POSED if posed else 0) | (ADAPT_CONTINUE if resume else 0)
        self._mean_call("rtx_render_view_adaptive_device", device, view, light, flags, seeds, n_pairs, rule=rule,
                        tail=(d_moments_ptr, d_tiles_ptr, d_rgb_ptr, d_shade_ptr, stream))

    # -- the adaptive mean through the render pipeline: a stopped tile is not scheduled (full width only, the same words)
    def render_view_rows_adaptive(self, view, seeds, rule, n_pairs=NB_RAND_SAMPLE, device=0, light=None, posed=False, stats=False,
                                  want_shade=False, want_tiles=False):
        """render_view_adaptive through the render pipeline (rtx_render_view_rows_adaptive): the view's full-width rows, the
        pipeline's record launch behind the tile states in the masked view kernel's place; every output is
        render_view_adaptive's, word for word."""
        return self._mean_call("rtx_render_view_rows_adaptive", device, view, light, MEAN_POSED if posed else 0, seeds, n_pairs,
                               rule=rule, want=(want_shade, want_tiles, stats))

    def render_view_rows_adaptive_device(self, device, view, seeds, rule, n_pairs, d_moments_ptr, d_tiles_ptr, d_rgb_ptr=None,
                                         d_shade_ptr=None, stream=None, light=None, posed=False, resume=False):
        """Asynchronous: render_view_adaptive_device through the render pipeline (rtx_render_view_rows_adaptive_device), the
        same buffers and the same words."""
        flags = (MEAN_POSED if posed else 0) | (ADAPT_CONTINUE if resume else 0)
        self._mean_call("rtx_render_view_rows_adaptive_device", device, view, light, flags, seeds, n_pairs, rule=rule,
                        tail=(d_moments_ptr, d_tiles_ptr, d_rgb_ptr, d_shade_ptr, stream))

    def render_view_rows_shade_masked_device(self, device, view, d_tiles_ptr, rule, d_shade_ptr, d_bytes, stream=None,
                                             d_counters_ptr=None, light=None, posed=False):
        """Asynchronous: render_view_rows_shade_device behind a tile mask (rtx_render_view_rows_shade_masked_device) — d_tiles_ptr:
        tiles_y*tiles_x x 8 bytes of tile states (8-byte aligned); a tile stopped under `rule` is not scheduled and its
        records in d_shade keep their words, a live tile's records are the unmasked launch's."""
        r = AdaptRule(int(rule[0]), float(rule[1])) if rule is not None else None
        _check(_lib.rtx_render_view_rows_shade_masked_device(self._h, device, C.byref(view), C.byref(light) if light is not None else None,
                                                             ROWS_POSED if posed else 0, C.c_void_p(d_tiles_ptr) if d_tiles_ptr else None,
                                                             C.byref(r) if r is not None else None, C.c_void_p(d_shade_ptr), d_bytes,
                                                             C.c_void_p(stream) if stream else None,
                                                             C.c_void_p(d_counters_ptr) if d_counters_ptr else None),
               "rtx_render_view_rows_shade_masked_device")

    def moment_add_device(self, device, nx, ny, d_shade_ptr, d_moments_ptr, d_tiles_ptr, first, rule=None, stream=None):
        """Asynchronous: adds the nx x ny RtxPixelShade records of a rectangle — of any call that writes them — into its moment
        records, tile by tile, skipping the tiles that are stopped under `rule` (rtx_moment_add_device).  d_tiles_ptr None:
        every tile is live and no state is written.  first: moments and states are written, never read."""
        r = AdaptRule(int(rule[0]), float(rule[1])) if rule is not None else None
        _check(_lib.rtx_moment_add_device(self._h, device, int(nx), int(ny), C.c_void_p(d_shade_ptr), C.c_void_p(d_moments_ptr),
                                          C.c_void_p(d_tiles_ptr) if d_tiles_ptr else None, 1 if first else 0,
                                          C.byref(r) if r is not None else None,
                                          C.c_void_p(stream) if stream else None), "rtx_moment_add_device")

    def moment_resolve_device(self, device, n, d_moments_ptr, d_rgb_ptr=None, d_shade_ptr=None, stream=None):
        """Asynchronous: n moment records into n*3 bytes (any alignment) and / or n records (rtx_moment_resolve_device), each
        divided by its own frame count, through the scene's gamma thresholds."""
        _check(_lib.rtx_moment_resolve_device(self._h, device, int(n), C.c_void_p(d_moments_ptr),
                                              C.c_void_p(d_rgb_ptr) if d_rgb_ptr else None,
                                              C.c_void_p(d_shade_ptr) if d_shade_ptr else None,
                                              C.c_void_p(stream) if stream else None), "rtx_moment_resolve_device")


def default_scene(obj_paths, width=DEFAULT_WIDTH, height=DEFAULT_HEIGHT, samples=None, **kw):
    """The scene main() renders (src/main.rs:319-362) for the given OBJ files."""
    tris, rgb = default_primitives(obj_paths)
    if samples is None:
        samples = gen_samples()
    return Scene(width, height, tris, rgb, samples, **kw)


def tile_owner(tile, world_size):
    """Row tile -> rank (interleaved): tile t belongs to rank t % world_size."""
    return tile % world_size


def scatter_tiles(frame, packed, first_tile, tile_stride, tile_rows):
    """Place the packed rows of rtx_render_tiles_device back into a [H, W, 3] frame (rtxh_scatter_tiles: the loop
    rtx_render_frame itself gathers with)."""
    h, w = frame.shape[0], frame.shape[1]
    assert frame.flags["C_CONTIGUOUS"] and frame.dtype == np.uint8
    packed = np.ascontiguousarray(packed, dtype=np.uint8)
    assert packed.size == tiles_rows_of(h, first_tile, tile_stride, tile_rows) * w * 3, "packed share has the wrong size"
    _check(_lib.rtxh_scatter_tiles(frame.ctypes.data, h, w, packed.ctypes.data, first_tile, tile_stride, tile_rows),
           "rtxh_scatter_tiles")
    return frame


def tiles_rows_of(height, first_tile, tile_stride, tile_rows):
    """Rows of the share (first_tile, tile_stride, tile_rows) of a frame of `height` rows."""
    rows, t = 0, first_tile
    while t * tile_rows < height:
        rows += min(tile_rows, height - t * tile_rows)
        t += tile_stride
    return rows
