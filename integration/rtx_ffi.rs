//! src/rtx_ffi.rs — binding of librtx.so (include/rtx.h, RTX_ABI_VERSION 3) for the reference crate.
//!
//! Mirrors the header declaration by declaration.  The `#[repr(C)]` structs below are checked against the C header
//! WITHOUT a Rust toolchain: tests/test_ffi_layout.py parses this file, lays the fields out by the C rules, and
//! compares every offset and size with what a C compiler reports for include/rtx.h (integration/layout.json is the
//! table both sides must equal).  Edit the header, this file and the table together.
#![allow(dead_code)]
use std::ffi::CStr;
use std::os::raw::{c_char, c_int, c_void};

pub const RTX_ABI_VERSION: c_int = 3;
pub const RTX_OK: c_int = 0;

/// One entry of the random-sample table.  `Vec<(f32, f32)>` (src/main.rs:253) has NO guaranteed layout — Rust tuples
/// are `repr(Rust)` — so the table handed to the library is a `Vec<Sample>` (or a `Vec<[f32; 2]>`): two packed f32.
#[repr(C)]
#[derive(Clone, Copy, Default)]
pub struct Sample {
    pub s0: f32,
    pub s1: f32,
}

#[repr(C)]
pub struct RtxSceneDesc {
    pub width: u32,
    pub height: u32,
    pub eye: [f32; 3],
    pub u: [f32; 3],
    pub v: [f32; 3],
    pub w: [f32; 3],
    pub distance: f32,
    pub light_v0: [f32; 3],
    pub light_v1: [f32; 3],
    pub light_v2: [f32; 3],
    pub n_tris: u32,
    pub v0v1v2: *const f32,
    pub rgb: *const f32,
    pub tie_rank: *const u32,
    pub nb_ray: u32,
    pub nb_light_sample: u32,
    pub samples: *const f32,
    pub n_samples: u32,
    pub accel: u32,
    pub leaf_max: u32,
    pub reference_tree: u32,
    pub n_spheres: u32,
    pub spheres: *const f32,
    pub sphere_rgb: *const f32,
    pub kinds: *const u8,
}

#[repr(C)]
#[derive(Default)]
pub struct RtxStats {
    pub primary_rays: u64,
    pub primary_hits: u64,
    pub shadow_rays: u64,
    pub rays: u64,
    pub box_tests: u64,
    pub tri_tests: u64,
    pub wave_node_visits: u64,
    pub wave_tri_visits: u64,
    pub redo_tiles: u64,
    pub kernel_ms: f64,
    pub total_ms: f64,
}

#[repr(C)]
#[derive(Default)]
pub struct RtxSceneInfo {
    pub n_tris: u32,
    pub n_nodes: u32,
    pub n_leaves: u32,
    pub max_leaf_tris: u32,
    pub depth: u32,
    pub n_light_points: u32,
    pub n_ref_nodes: u32,
    pub n_global: u32,
    pub node_bytes: u64,
    pub tri_bytes: u64,
    pub shade_bytes: u64,
    pub sample_bytes: u64,
}

/// One closest hit of `rtx_trace_rays`: what `BoundingVolumeHierarchy::intersect` returns as `Option<HitInfo>`,
/// flattened (`prim == RTX_NO_HIT` is `None`; colour is the caller's own `rgb[prim]`).
#[repr(C)]
#[derive(Default, Clone, Copy)]
pub struct RtxRayHit {
    pub prim: u32,
    pub t: f32,
    pub p_hit: [f32; 3],
    pub normal: [f32; 3],
}
/// One pixel of `rtx_shade_rays`: `render_pixel`'s `avg_col` for the caller's rays, its `Color::to_rgba` bytes, and how
/// many of the pixel's `nb_ray` rays had a closest hit (saturating at 255).
#[repr(C)]
#[derive(Default, Clone, Copy)]
pub struct RtxPixelShade {
    pub linear: [f32; 3],
    pub rgb8: [u8; 3],
    pub hits: u8,
}
/// One pixel of an accumulator of `rtx_render_view_mean` / `rtx_accum_add_device`: the ordered f32 sum of the frames'
/// linear colours and in how many frames the pixel had a closest hit.  A device array of them must be 16-byte aligned.
#[repr(C)]
#[derive(Default, Clone, Copy)]
pub struct RtxAccumPixel {
    pub sum: [f32; 3],
    pub hit_frames: u32,
}
/// A pixel of the adaptive mean (`rtx_render_view_adaptive`): `RtxAccumPixel`'s words, the ordered `f32` sum of the frames'
/// squared linear colours and the frames this pixel received.  A device array of them must be 16-byte aligned.
#[repr(C)]
#[derive(Default, Clone, Copy)]
pub struct RtxMomentPixel {
    pub sum: [f32; 3],
    pub hit_frames: u32,
    pub sumsq: [f32; 3],
    pub frames: u32,
}
/// An 8 x 8 tile of the rectangle: the frames it received and its noise estimate after its last add.  A device array of
/// them must be 8-byte aligned.
#[repr(C)]
#[derive(Default, Clone, Copy)]
pub struct RtxTileState {
    pub frames: u32,
    pub err: f32,
}
/// A tile is stopped when `frames >= min_frames && err <= max_variance`.  `min_frames == 1` stops every tile after one
/// frame, whose variance is exactly 0: `min_frames >= 2` is the meaningful range.
#[repr(C)]
#[derive(Default, Clone, Copy)]
pub struct RtxAdaptRule {
    pub min_frames: u32,
    pub max_variance: f32,
}
pub const RTX_ADAPT_CONTINUE: u32 = 2;
pub const RTX_MEAN_POSED: u32 = 1;
pub const RTX_ROWS_POSED: u32 = 1;
pub const RTX_MAX_MEAN_FRAMES: u32 = 65536;
/// A pinhole view of an uploaded scene for `rtx_render_view`: the frame `create_rays` sees, the `Camera` after
/// `Camera::new` (`rtxh_camera_new` computes `u`, `v`, `w`) and the rectangle of pixels to render.
#[repr(C)]
#[derive(Default, Clone, Copy)]
pub struct RtxView {
    pub width: u32,
    pub height: u32,
    pub eye: [f32; 3],
    pub u: [f32; 3],
    pub v: [f32; 3],
    pub w: [f32; 3],
    pub distance: f32,
    pub x0: u32,
    pub y0: u32,
    pub nx: u32,
    pub ny: u32,
}
/// The area light of one lit call (`rtx_render_view_lit`, `rtx_shade_rays_lit`): the vertices of `Light.primitives[0]`,
/// the triangle `get_sample` samples, and `NB_LIGHT_SAMPLE` for the call (0 = the scene's).  40 bytes, alignment 4.
#[repr(C)]
#[derive(Default, Clone, Copy)]
pub struct RtxLight {
    pub v0: [f32; 3],
    pub v1: [f32; 3],
    pub v2: [f32; 3],
    pub nb_light_sample: u32,
}
/// What `rtx_scene_pose_prims` states: host pointers for the host variant, device pointers for `_device`.  `v0v1v2` is
/// required when the scene has triangles; a NULL `spheres` (`n_spheres x 4`: origin, radius), `rgb` (`n_tris x 3`) or
/// `sphere_rgb` (`n_spheres x 3`) means "as uploaded"; `tie_rank` as `rtx_scene_pose`'s.
#[repr(C)]
#[derive(Clone, Copy)]
pub struct RtxPosePrims {
    pub v0v1v2: *const f32,
    pub spheres: *const f32,
    pub rgb: *const f32,
    pub sphere_rgb: *const f32,
    pub tie_rank: *const u32,
}
pub const RTX_POSE_REBUILT: u32 = 1;
/// What `rtx_scene_pose_moved` states: `n_moves` (1 ..= 65,536) affine maps of 12 floats (3 x 4, row major: a row of A, then
/// that row's translation), the move each Vec position follows (`group`: NULL = all follow move 0, `RTX_MOVE_NONE` = the
/// primitive keeps its created words), a factor per move for a sphere's radius (`radius_scale`, NULL = as uploaded), and
/// `rgb` / `sphere_rgb` / `tie_rank` as `RtxPosePrims`'.  Host pointers for the host variant, device pointers for `_device`.
#[repr(C)]
#[derive(Clone, Copy)]
pub struct RtxPoseMoves {
    pub n_moves: u32,
    pub moves: *const f32,
    pub group: *const u32,
    pub radius_scale: *const f32,
    pub rgb: *const f32,
    pub sphere_rgb: *const f32,
    pub tie_rank: *const u32,
}
pub const RTX_MOVE_NONE: u32 = 0xFFFF_FFFF;
/// What `rtx_scene_skin` binds (host pointers, copied by the call): per triangle corner four move indices and four weights
/// (`n_triangles x 3 x 4` each, corners in `RtxSceneDesc.v0v1v2` order), per sphere one move index (`sphere_bone`: NULL =
/// every sphere `RTX_MOVE_NONE`).  The scene keeps 96 bytes per triangle.
#[repr(C)]
#[derive(Clone, Copy)]
pub struct RtxSkin {
    pub bones: *const u32,
    pub weights: *const f32,
    pub sphere_bone: *const u32,
}
pub const RTX_NO_HIT: u32 = 0xFFFF_FFFF;
pub const RTX_RAYS_KEEP_ORDER: u32 = 1;
pub const RTX_RAYS_FORCE_REGROUP: u32 = 2;

/// Opaque handle (library-owned).
#[repr(C)]
pub struct RtxScene {
    _private: [u8; 0],
}

extern "C" {
    pub fn rtx_abi_version() -> c_int;
    pub fn rtx_device_count() -> c_int;
    pub fn rtx_scene_create(desc: *const RtxSceneDesc, out: *mut *mut RtxScene) -> c_int;
    pub fn rtx_scene_destroy(scene: *mut RtxScene);
    pub fn rtx_scene_info(scene: *const RtxScene, info: *mut RtxSceneInfo) -> c_int;
    pub fn rtx_scene_upload(scene: *mut RtxScene, device: c_int) -> c_int;
    pub fn rtx_render_rows(scene: *mut RtxScene, device: c_int, row0: u32, nrows: u32, out_rgb: *mut u8,
                           stats: *mut RtxStats) -> c_int;
    pub fn rtx_render_frame(scene: *mut RtxScene, devices: *const c_int, n_devices: c_int, tile_rows: u32,
                            out_rgb: *mut u8, stats: *mut RtxStats) -> c_int;
    pub fn rtx_render_tiles_device(scene: *mut RtxScene, device: c_int, first_tile: u32, tile_stride: u32,
                                   tile_rows: u32, d_out_rgb: *mut c_void, d_out_bytes: usize, stream: *mut c_void,
                                   d_counters: *mut u64) -> c_int;
    pub fn rtx_tiles_rows(scene: *const RtxScene, first_tile: u32, tile_stride: u32, tile_rows: u32) -> u32;
    pub fn rtx_tiles_bytes(scene: *const RtxScene, first_tile: u32, tile_stride: u32, tile_rows: u32) -> usize;
    pub fn rtx_trace_rays(scene: *mut RtxScene, device: c_int, n_rays: u32, origins: *const f32, directions: *const f32,
                          flags: u32, out_hits: *mut RtxRayHit, stats: *mut RtxStats) -> c_int;
    pub fn rtx_occluded_rays(scene: *mut RtxScene, device: c_int, n_rays: u32, origins: *const f32, targets: *const f32,
                             flags: u32, out_occluded: *mut u8, stats: *mut RtxStats) -> c_int;
    pub fn rtx_trace_rays_device(scene: *mut RtxScene, device: c_int, n_rays: u32, d_origins: *const c_void,
                                 d_directions: *const c_void, flags: u32, d_hits: *mut c_void, stream: *mut c_void) -> c_int;
    pub fn rtx_occluded_rays_device(scene: *mut RtxScene, device: c_int, n_rays: u32, d_origins: *const c_void,
                                    d_targets: *const c_void, flags: u32, d_occluded: *mut c_void, stream: *mut c_void) -> c_int;
    pub fn rtx_shade_rays(scene: *mut RtxScene, device: c_int, n_pixels: u32, origins: *const f32, directions: *const f32,
                          flags: u32, out_shade: *mut RtxPixelShade, out_hits: *mut RtxRayHit, stats: *mut RtxStats) -> c_int;
    pub fn rtx_shade_rays_device(scene: *mut RtxScene, device: c_int, n_pixels: u32, d_origins: *const c_void,
                                 d_directions: *const c_void, flags: u32, d_shade: *mut c_void, d_hits: *mut c_void,
                                 stream: *mut c_void) -> c_int;
    pub fn rtx_scene_view(scene: *const RtxScene, out: *mut RtxView) -> c_int;
    pub fn rtx_render_view(scene: *mut RtxScene, device: c_int, view: *const RtxView, out_rgb: *mut u8,
                           out_shade: *mut RtxPixelShade, out_hits: *mut RtxRayHit, stats: *mut RtxStats) -> c_int;
    pub fn rtx_render_view_device(scene: *mut RtxScene, device: c_int, view: *const RtxView, d_rgb: *mut c_void,
                                  d_shade: *mut c_void, d_hits: *mut c_void, stream: *mut c_void) -> c_int;
    /// Rows `[y0, y0 + ny)` of the view through the render pipeline, full width (`x0 == 0`, `nx == width`): `rtx_render_view`'s
    /// bytes at `rtx_render_rows`' speed.  `RTX_ERR_UNSUPPORTED` (-5) for an eye beyond the scene's largest coordinate.
    pub fn rtx_render_view_rows(scene: *mut RtxScene, device: c_int, view: *const RtxView, out_rgb: *mut u8,
                                stats: *mut RtxStats) -> c_int;
    pub fn rtx_render_view_rows_device(scene: *mut RtxScene, device: c_int, view: *const RtxView, d_rgb: *mut c_void,
                                       d_bytes: usize, stream: *mut c_void, d_counters: *mut u64) -> c_int;
    /// The light and sample count `rtx_scene_create` was given.
    pub fn rtx_scene_light(scene: *const RtxScene, out: *mut RtxLight) -> c_int;
    /// `rtx_render_view` / `rtx_shade_rays` (and their device-resident forms) under another light: no new scene.  A NULL
    /// light or more than 2^20 light points: `RTX_ERR_BAD_ARG`; a vertex that is not finite: `RTX_ERR_UNSUPPORTED` (-5).
    /// Device-resident lit launches on one device must be ordered on one stream (one library-owned light buffer).
    pub fn rtx_render_view_lit(scene: *mut RtxScene, device: c_int, view: *const RtxView, light: *const RtxLight,
                               out_rgb: *mut u8, out_shade: *mut RtxPixelShade, out_hits: *mut RtxRayHit,
                               stats: *mut RtxStats) -> c_int;
    pub fn rtx_render_view_lit_device(scene: *mut RtxScene, device: c_int, view: *const RtxView, light: *const RtxLight,
                                      d_rgb: *mut c_void, d_shade: *mut c_void, d_hits: *mut c_void,
                                      stream: *mut c_void) -> c_int;
    pub fn rtx_shade_rays_lit(scene: *mut RtxScene, device: c_int, n_pixels: u32, origins: *const f32,
                              directions: *const f32, flags: u32, light: *const RtxLight, out_shade: *mut RtxPixelShade,
                              out_hits: *mut RtxRayHit, stats: *mut RtxStats) -> c_int;
    pub fn rtx_shade_rays_lit_device(scene: *mut RtxScene, device: c_int, n_pixels: u32, d_origins: *const c_void,
                                     d_directions: *const c_void, flags: u32, light: *const RtxLight, d_shade: *mut c_void,
                                     d_hits: *mut c_void, stream: *mut c_void) -> c_int;
    /// Posing: the uploaded scene's triangles moved to `v0v1v2` (`n_tris x 9` floats, Vec order, spheres skipped) on
    /// `device`: one pose per scene and device, replaced by the next.  Every coordinate must be finite and at most
    /// `rtx_scene_pose_bound`'s value in magnitude (`RTX_ERR_UNSUPPORTED`).  `tie_rank` may be NULL.
    pub fn rtx_scene_pose_bound(scene: *const RtxScene, out_magnitude: *mut f32) -> c_int;
    pub fn rtx_scene_pose(scene: *mut RtxScene, device: c_int, v0v1v2: *const f32, tie_rank: *const u32, reference_tree: u32,
                          stats: *mut RtxStats) -> c_int;
    pub fn rtx_scene_pose_device(scene: *mut RtxScene, device: c_int, d_v0v1v2: *const c_void, d_tie_rank: *const c_void,
                                 stream: *mut c_void) -> c_int;
    /// The posed calls: their unposed twins against the device's pose; `light` NULL = the scene's, else the `_lit` twin.
    pub fn rtx_trace_rays_posed(scene: *mut RtxScene, device: c_int, n_rays: u32, origins: *const f32, directions: *const f32,
                                flags: u32, out_hits: *mut RtxRayHit, stats: *mut RtxStats) -> c_int;
    pub fn rtx_occluded_rays_posed(scene: *mut RtxScene, device: c_int, n_rays: u32, origins: *const f32, targets: *const f32,
                                   flags: u32, out_occluded: *mut u8, stats: *mut RtxStats) -> c_int;
    pub fn rtx_trace_rays_posed_device(scene: *mut RtxScene, device: c_int, n_rays: u32, d_origins: *const c_void,
                                       d_directions: *const c_void, flags: u32, d_hits: *mut c_void,
                                       stream: *mut c_void) -> c_int;
    pub fn rtx_occluded_rays_posed_device(scene: *mut RtxScene, device: c_int, n_rays: u32, d_origins: *const c_void,
                                          d_targets: *const c_void, flags: u32, d_occluded: *mut c_void,
                                          stream: *mut c_void) -> c_int;
    pub fn rtx_shade_rays_posed(scene: *mut RtxScene, device: c_int, n_pixels: u32, origins: *const f32, directions: *const f32,
                                flags: u32, light: *const RtxLight, out_shade: *mut RtxPixelShade, out_hits: *mut RtxRayHit,
                                stats: *mut RtxStats) -> c_int;
    pub fn rtx_shade_rays_posed_device(scene: *mut RtxScene, device: c_int, n_pixels: u32, d_origins: *const c_void,
                                       d_directions: *const c_void, flags: u32, light: *const RtxLight, d_shade: *mut c_void,
                                       d_hits: *mut c_void, stream: *mut c_void) -> c_int;
    pub fn rtx_render_view_posed(scene: *mut RtxScene, device: c_int, view: *const RtxView, light: *const RtxLight,
                                 out_rgb: *mut u8, out_shade: *mut RtxPixelShade, out_hits: *mut RtxRayHit,
                                 stats: *mut RtxStats) -> c_int;
    pub fn rtx_render_view_posed_device(scene: *mut RtxScene, device: c_int, view: *const RtxView, light: *const RtxLight,
                                        d_rgb: *mut c_void, d_shade: *mut c_void, d_hits: *mut c_void,
                                        stream: *mut c_void) -> c_int;
    /// Host only: the words the pose kernels make (each output may be NULL); `rtx_debug_pose` reads the device's back.
    pub fn rtx_scene_posed_records(scene: *const RtxScene, v0v1v2: *const f32, tie_rank: *const u32, out_tris: *mut u32,
                                   out_shade: *mut u32, out_nodes: *mut u32) -> c_int;
    pub fn rtx_debug_pose(scene: *mut RtxScene, device: c_int, out_tris: *mut u32, out_shade: *mut u32,
                          out_nodes: *mut u32) -> c_int;
    /// The pose through the render pipeline: `rtx_render_view_rows` / `_device` (NULL light) or `rtx_render_view_rows_lit`
    /// / `_device` with the device's pose in place of the uploaded triangles; `RTX_ERR_BAD_ARG` when it holds none.
    pub fn rtx_render_view_rows_posed(scene: *mut RtxScene, device: c_int, view: *const RtxView, light: *const RtxLight,
                                      out_rgb: *mut u8, stats: *mut RtxStats) -> c_int;
    pub fn rtx_render_view_rows_posed_device(scene: *mut RtxScene, device: c_int, view: *const RtxView, light: *const RtxLight,
                                             d_rgb: *mut c_void, d_bytes: usize, stream: *mut c_void,
                                             d_counters: *mut u64) -> c_int;
    /// The pipeline's linear output: the rows as `RtxPixelShade` records, `rtx_render_view_lit`'s (with `RTX_ROWS_POSED`
    /// `rtx_render_view_posed`'s) `out_shade` bit for bit; otherwise the byte twin chosen by `light` and `flags`.
    /// `d_shade`: 16-byte aligned, `d_bytes >= ny * width * 16`; an unknown flag is `RTX_ERR_BAD_ARG`.
    pub fn rtx_render_view_rows_shade(scene: *mut RtxScene, device: c_int, view: *const RtxView, light: *const RtxLight,
                                      flags: u32, out_shade: *mut RtxPixelShade, stats: *mut RtxStats) -> c_int;
    pub fn rtx_render_view_rows_shade_device(scene: *mut RtxScene, device: c_int, view: *const RtxView, light: *const RtxLight,
                                             flags: u32, d_shade: *mut c_void, d_bytes: usize, stream: *mut c_void,
                                             d_counters: *mut u64) -> c_int;
    /// `rtx_render_view_mean` / `_device` through the render pipeline: full width only, the same outputs and accumulator word
    /// for word; the eye's range rule and every frame's shaft margin are decided on the host (`RTX_ERR_UNSUPPORTED`).
    pub fn rtx_render_view_rows_mean(scene: *mut RtxScene, device: c_int, view: *const RtxView, light: *const RtxLight, flags: u32,
                                     seeds: *const u64, n_frames: u32, n_pairs: u32, out_rgb: *mut u8,
                                     out_shade: *mut RtxPixelShade, stats: *mut RtxStats) -> c_int;
    pub fn rtx_render_view_rows_mean_device(scene: *mut RtxScene, device: c_int, view: *const RtxView, light: *const RtxLight,
                                            flags: u32, seeds: *const u64, n_frames: u32, n_pairs: u32, d_accum: *mut c_void,
                                            d_rgb: *mut c_void, d_shade: *mut c_void, stream: *mut c_void) -> c_int;
    /// Host only: the adaptive mean's add over an `nx` x `ny` rectangle, tile by tile: the tiles that are stopped under
    /// `rule` are skipped.  `tiles` NULL (`rule` may be too): every tile is live, no state is written.
    pub fn rtxh_moment_add(nx: u32, ny: u32, shade: *const RtxPixelShade, moments: *mut RtxMomentPixel, tiles: *mut RtxTileState,
                           first: u32, rule: *const RtxAdaptRule) -> c_int;
    /// Host only: moment records into RGB8 (NULL or `n * 3` bytes) and records (NULL or `n`), each pixel divided by its own
    /// frame count.
    pub fn rtxh_moment_resolve(thr256: *const f32, n: u32, moments: *const RtxMomentPixel, out_rgb: *mut u8,
                               out_shade: *mut RtxPixelShade) -> c_int;
    /// The add over device arrays (records and moments 16-byte, tile states 8-byte aligned), asynchronous on `stream`.
    pub fn rtx_moment_add_device(scene: *mut RtxScene, device: c_int, nx: u32, ny: u32, d_shade: *const c_void,
                                 d_moments: *mut c_void, d_tiles: *mut c_void, first: u32, rule: *const RtxAdaptRule,
                                 stream: *mut c_void) -> c_int;
    /// The resolve over device moments; `d_rgb` may have any alignment.
    pub fn rtx_moment_resolve_device(scene: *mut RtxScene, device: c_int, n: u32, d_moments: *const c_void, d_rgb: *mut c_void,
                                     d_shade: *mut c_void, stream: *mut c_void) -> c_int;
    /// `rtx_render_view_mean` whose 8 x 8 tiles stop receiving frames once `rule` is met; `out_tiles` (may be NULL): the
    /// tile states after the last frame.  The scene is not changed.
    pub fn rtx_render_view_adaptive(scene: *mut RtxScene, device: c_int, view: *const RtxView, light: *const RtxLight, flags: u32,
                                    seeds: *const u64, n_frames: u32, n_pairs: u32, rule: *const RtxAdaptRule, out_rgb: *mut u8,
                                    out_shade: *mut RtxPixelShade, out_tiles: *mut RtxTileState, stats: *mut RtxStats) -> c_int;
    /// Device-resident variant: the caller's moments, tile states, outputs and stream.  `flags`: `RTX_MEAN_POSED |
    /// RTX_ADAPT_CONTINUE` — continue: the moments and states are an earlier call's, `seeds` the next frames'.
    pub fn rtx_render_view_adaptive_device(scene: *mut RtxScene, device: c_int, view: *const RtxView, light: *const RtxLight,
                                           flags: u32, seeds: *const u64, n_frames: u32, n_pairs: u32, rule: *const RtxAdaptRule,
                                           d_moments: *mut c_void, d_tiles: *mut c_void, d_rgb: *mut c_void, d_shade: *mut c_void,
                                           stream: *mut c_void) -> c_int;
    /// `rtx_render_view_adaptive` / `_device` through the render pipeline: full width only, every output word for word; a
    /// stopped tile is not scheduled.  The eye's range rule and every frame's shaft margin are decided on the host.
    pub fn rtx_render_view_rows_adaptive(scene: *mut RtxScene, device: c_int, view: *const RtxView, light: *const RtxLight, flags: u32,
                                         seeds: *const u64, n_frames: u32, n_pairs: u32, rule: *const RtxAdaptRule, out_rgb: *mut u8,
                                         out_shade: *mut RtxPixelShade, out_tiles: *mut RtxTileState, stats: *mut RtxStats) -> c_int;
    pub fn rtx_render_view_rows_adaptive_device(scene: *mut RtxScene, device: c_int, view: *const RtxView, light: *const RtxLight,
                                                flags: u32, seeds: *const u64, n_frames: u32, n_pairs: u32, rule: *const RtxAdaptRule,
                                                d_moments: *mut c_void, d_tiles: *mut c_void, d_rgb: *mut c_void, d_shade: *mut c_void,
                                                stream: *mut c_void) -> c_int;
    /// `rtx_render_view_rows_shade_device` behind a tile mask: a tile stopped under `rule` by its state in `d_tiles` (8-byte
    /// aligned, tiles row by row) is not scheduled and its records in `d_shade` keep their words.
    pub fn rtx_render_view_rows_shade_masked_device(scene: *mut RtxScene, device: c_int, view: *const RtxView, light: *const RtxLight,
                                                    flags: u32, d_tiles: *const c_void, rule: *const RtxAdaptRule, d_shade: *mut c_void,
                                                    d_bytes: usize, stream: *mut c_void, d_counters: *mut u64) -> c_int;
    /// Host only: `rtx_scene_light_walk_for`'s outputs on a scene reseeded with (`seed`, `n_pairs`); `light` NULL: the scene's.
    pub fn rtx_scene_light_walk_seeded(scene: *const RtxScene, light: *const RtxLight, seed: u64, n_pairs: u32,
                                       out_order: *mut u32, out_boxes: *mut f32, out_shaft_delta: *mut f32) -> c_int;
    /// Host only: the plane records (n_global x 16 words) and the aimed stream (n_nodes x 8 words) a pose makes for the
    /// pipeline; each output may be NULL, `eye` when `out_aimed` is.  `rtx_debug_pose_pipeline` reads the device's back.
    pub fn rtx_scene_posed_pipeline_records(scene: *const RtxScene, v0v1v2: *const f32, eye: *const f32, out_planes: *mut u32,
                                            out_aimed: *mut u32) -> c_int;
    pub fn rtx_debug_pose_pipeline(scene: *mut RtxScene, device: c_int, eye: *const f32, out_planes: *mut u32,
                                   out_aimed: *mut u32) -> c_int;
    /// A pose whose tree is rebuilt on the device: `rtx_scene_pose` / `_device` in every respect except the tree — the
    /// tree proper's records sorted by a 64-bit Morton key, a balanced tree over the sorted runs, boxes by the refit.
    /// Every posed call then runs over it unchanged.
    pub fn rtx_scene_pose_rebuilt(scene: *mut RtxScene, device: c_int, v0v1v2: *const f32, tie_rank: *const u32,
                                  reference_tree: u32, stats: *mut RtxStats) -> c_int;
    pub fn rtx_scene_pose_rebuilt_device(scene: *mut RtxScene, device: c_int, d_v0v1v2: *const c_void, d_tie_rank: *const c_void,
                                         stream: *mut c_void) -> c_int;
    /// Host only: the rebuilt stream's node count, and the words a rebuilt pose makes (each output may be NULL).
    pub fn rtx_scene_rebuilt_counts(scene: *const RtxScene, out_n_nodes: *mut u32) -> c_int;
    pub fn rtx_scene_rebuilt_records(scene: *const RtxScene, v0v1v2: *const f32, tie_rank: *const u32, out_keys: *mut u64,
                                     out_perm: *mut u32, out_tris: *mut u32, out_shade: *mut u32, out_nodes: *mut u32) -> c_int;
    pub fn rtx_scene_rebuilt_aimed(scene: *const RtxScene, v0v1v2: *const f32, eye: *const f32, out_aimed: *mut u32) -> c_int;
    /// Diagnostic: the rebuilt pose the device holds, and the aim kernels' output over it for `eye`; blocks.
    pub fn rtx_debug_pose_rebuilt(scene: *mut RtxScene, device: c_int, eye: *const f32, out_perm: *mut u32, out_tris: *mut u32,
                                  out_shade: *mut u32, out_nodes: *mut u32, out_aimed: *mut u32) -> c_int;
    /// A pose that states every field of a primitive: `rtx_scene_pose` / `_device` (flags 0) or `rtx_scene_pose_rebuilt`
    /// / `_device` (`RTX_POSE_REBUILT`) with the spheres' origins and radii and both arms' colours stated too; NULL
    /// arrays are as uploaded.  A sphere's box words beyond `rtx_scene_pose_bound`: `RTX_ERR_UNSUPPORTED` (host variant).
    pub fn rtx_scene_pose_prims(scene: *mut RtxScene, device: c_int, prims: *const RtxPosePrims, flags: u32,
                                reference_tree: u32, stats: *mut RtxStats) -> c_int;
    pub fn rtx_scene_pose_prims_device(scene: *mut RtxScene, device: c_int, prims: *const RtxPosePrims, flags: u32,
                                       stream: *mut c_void) -> c_int;
    /// Host only: the words such a pose makes, in `rtx_scene_posed_records`' layout (flags 0: `out_keys` and `out_perm`
    /// must be NULL) or `rtx_scene_rebuilt_records`'; and the aim kernels' output over it for `eye`.
    pub fn rtx_scene_pose_prims_records(scene: *const RtxScene, prims: *const RtxPosePrims, flags: u32, out_keys: *mut u64,
                                        out_perm: *mut u32, out_tris: *mut u32, out_shade: *mut u32, out_nodes: *mut u32) -> c_int;
    pub fn rtx_scene_pose_prims_aimed(scene: *const RtxScene, prims: *const RtxPosePrims, flags: u32, eye: *const f32,
                                      out_aimed: *mut u32) -> c_int;
    /// A pose whose vertices and spheres the DEVICE makes from the scene's geometry as created and `moves`: everything else
    /// is `rtx_scene_pose_prims` / `_device`.  A group value that is neither below `n_moves` nor `RTX_MOVE_NONE`:
    /// `RTX_ERR_BAD_ARG` (host variant); moved primitives beyond `rtx_scene_pose_bound`: `RTX_ERR_UNSUPPORTED` (host variant).
    pub fn rtx_scene_pose_moved(scene: *mut RtxScene, device: c_int, moves: *const RtxPoseMoves, flags: u32,
                                reference_tree: u32, stats: *mut RtxStats) -> c_int;
    pub fn rtx_scene_pose_moved_device(scene: *mut RtxScene, device: c_int, moves: *const RtxPoseMoves, flags: u32,
                                       stream: *mut c_void) -> c_int;
    /// Host only: the `n_tris x 9` vertices and `n_spheres x 4` spheres such a pose makes (either may be NULL).
    pub fn rtx_scene_moved_prims(scene: *const RtxScene, moves: *const RtxPoseMoves, out_v0v1v2: *mut f32,
                                 out_spheres: *mut f32) -> c_int;
    /// Diagnostic: the same two arrays as the move or skin kernel last wrote them on `device`; blocks.
    pub fn rtx_debug_moved_prims(scene: *mut RtxScene, device: c_int, out_v0v1v2: *mut f32, out_spheres: *mut f32) -> c_int;
    /// Binds a skin to the scene (NULL: unbinds); host only, no device touched, not re-entrant per handle.
    /// `RTX_ERR_UNSUPPORTED`: a weight that is not finite.
    pub fn rtx_scene_skin(scene: *mut RtxScene, skin: *const RtxSkin) -> c_int;
    /// 1: a skin is bound, 0: none; `out_max_bone` (may be NULL): the largest bone other than `RTX_MOVE_NONE`.
    pub fn rtx_scene_skin_bound(scene: *const RtxScene, out_max_bone: *mut u32) -> c_int;
    /// `rtx_scene_pose_moved` / `_device` / `rtx_scene_moved_prims` with the bound skin naming the moves: every triangle
    /// corner blends up to four of them.  `moves.group` must be NULL and a skin bound, else `RTX_ERR_BAD_ARG`; host variant:
    /// also `RTX_ERR_BAD_ARG` when `n_moves` is not above the skin's largest bone.
    pub fn rtx_scene_pose_skinned(scene: *mut RtxScene, device: c_int, moves: *const RtxPoseMoves, flags: u32,
                                  reference_tree: u32, stats: *mut RtxStats) -> c_int;
    pub fn rtx_scene_pose_skinned_device(scene: *mut RtxScene, device: c_int, moves: *const RtxPoseMoves, flags: u32,
                                         stream: *mut c_void) -> c_int;
    pub fn rtx_scene_skinned_prims(scene: *const RtxScene, moves: *const RtxPoseMoves, out_v0v1v2: *mut f32,
                                   out_spheres: *mut f32) -> c_int;
    /// Replaces the scene's sample table by the caller's `n_samples` interleaved pairs (copied); host only, no device
    /// touched, not re-entrant per handle.  Light points, tour, boxes and shaft margin are re-derived as `rtx_scene_create`
    /// derives them; each device catches up in its next call.  `RTX_ERR_UNSUPPORTED`: a table `rtx_scene_create` would refuse.
    pub fn rtx_scene_resample(scene: *mut RtxScene, samples: *const f32, n_samples: u32) -> c_int;
    /// The same with the table `rtxh_gen_samples(seed, n_pairs)`, never made on the host: each device makes it from the seed.
    pub fn rtx_scene_reseed(scene: *mut RtxScene, seed: u64, n_pairs: u32) -> c_int;
    /// Host only: `count` pairs of the scene's current table from pair `first`.
    pub fn rtx_scene_samples(scene: *const RtxScene, first: u64, count: u32, out: *mut f32) -> c_int;
    /// Diagnostic: the same range of `device`'s table, after it caught up; blocks.
    pub fn rtx_debug_samples(scene: *mut RtxScene, device: c_int, first: u64, count: u32, out: *mut f32) -> c_int;
    /// Host only: frame records added into accumulator records (`first != 0`: written, never read), by the statement the
    /// device kernels compile too.
    pub fn rtxh_accum_add(n: u32, shade: *const RtxPixelShade, accum: *mut RtxAccumPixel, first: u32) -> c_int;
    /// Host only: accumulator records over `n_frames` frames into RGB8 (NULL or `n * 3` bytes) and records (NULL or `n`):
    /// one correctly rounded division per channel, then the byte through the scene's 256 gamma thresholds.
    pub fn rtxh_accum_resolve(thr256: *const f32, n: u32, accum: *const RtxAccumPixel, n_frames: u32, out_rgb: *mut u8,
                              out_shade: *mut RtxPixelShade) -> c_int;
    /// The add over device arrays (16-byte aligned), asynchronous on `stream`: records from any call that writes
    /// `RtxPixelShade`, so frames may differ in pose, eye or light.
    pub fn rtx_accum_add_device(scene: *mut RtxScene, device: c_int, n: u32, d_shade: *const c_void, d_accum: *mut c_void,
                                first: u32, stream: *mut c_void) -> c_int;
    /// The resolve over a device accumulator; `d_rgb` may have any alignment.
    pub fn rtx_accum_resolve_device(scene: *mut RtxScene, device: c_int, n: u32, d_accum: *const c_void, n_frames: u32,
                                    d_rgb: *mut c_void, d_shade: *mut c_void, stream: *mut c_void) -> c_int;
    /// The mean of `n_frames` frames of a view, frame `k` under the table `rtxh_gen_samples(seeds[k], n_pairs)`, summed in
    /// frame order on the device and divided once.  `light` NULL: the scene's.  `flags`: `RTX_MEAN_POSED` or 0.  The scene
    /// is not changed.
    pub fn rtx_render_view_mean(scene: *mut RtxScene, device: c_int, view: *const RtxView, light: *const RtxLight, flags: u32,
                                seeds: *const u64, n_frames: u32, n_pairs: u32, out_rgb: *mut u8,
                                out_shade: *mut RtxPixelShade, stats: *mut RtxStats) -> c_int;
    /// Device-resident variant: the caller's accumulator (`nx * ny` records), outputs and stream; nothing is waited for.
    pub fn rtx_render_view_mean_device(scene: *mut RtxScene, device: c_int, view: *const RtxView, light: *const RtxLight,
                                       flags: u32, seeds: *const u64, n_frames: u32, n_pairs: u32, d_accum: *mut c_void,
                                       d_rgb: *mut c_void, d_shade: *mut c_void, stream: *mut c_void) -> c_int;
    pub fn rtx_scene_light_points_for(scene: *const RtxScene, light: *const RtxLight, out: *mut f32) -> c_int;
    /// Diagnostic: the same points as the light kernel makes them on `device`.
    pub fn rtx_debug_light_points(scene: *mut RtxScene, device: c_int, light: *const RtxLight, out: *mut f32) -> c_int;
    /// `rtx_render_view_rows` / `_device` under another light: `rtx_render_view_lit`'s bytes at the pipeline's speed.  The
    /// twins' rules (full width, the eye's range) and the lit calls' (NULL light, 2^20 points, finite vertices); also
    /// `RTX_ERR_UNSUPPORTED` for a light `rtx_scene_create` would refuse (its shaft margin is not finite).
    pub fn rtx_render_view_rows_lit(scene: *mut RtxScene, device: c_int, view: *const RtxView, light: *const RtxLight,
                                    out_rgb: *mut u8, stats: *mut RtxStats) -> c_int;
    pub fn rtx_render_view_rows_lit_device(scene: *mut RtxScene, device: c_int, view: *const RtxView, light: *const RtxLight,
                                           d_rgb: *mut c_void, d_bytes: usize, stream: *mut c_void,
                                           d_counters: *mut u64) -> c_int;
    /// Host only: the walk order, boxes and shaft margin of `light` on this scene (each may be NULL); returns the point count.
    pub fn rtx_scene_light_walk_for(scene: *const RtxScene, light: *const RtxLight, out_order: *mut u32, out_boxes: *mut f32,
                                    out_shaft_delta: *mut f32) -> c_int;
    /// Diagnostic: the tour records and boxes as the light kernels make them on `device`.
    pub fn rtx_debug_light_walk(scene: *mut RtxScene, device: c_int, light: *const RtxLight, out_tour: *mut f32,
                                out_boxes: *mut f32) -> c_int;
    pub fn rtx_launch_timings(scene: *mut RtxScene, device: c_int, max_launches: c_int, schedule_ms: *mut f32,
                              shade_ms: *mut f32) -> c_int;
    /// The long primary walks (include/rtx.h): the scene's long list, one tile's weight and met records, and the
    /// debug switch (0 = predicted, 1 = no tile long, 2 = every tile long).
    pub fn rtx_scene_probe_long(scene: *const RtxScene, out_tiles: *mut u32, out_weights: *mut u32, max_entries: usize,
                                out_threshold: *mut u32) -> c_int;
    pub fn rtx_scene_probe_tile(scene: *const RtxScene, tile_x: u32, tile_y: u32, out_met: *mut u8,
                                out_weight: *mut u32) -> c_int;
    pub fn rtx_debug_probe_split(scene: *mut RtxScene, mode: u32) -> c_int;
    pub fn rtx_debug_probe_records(scene: *mut RtxScene, device: c_int, out_hits: *mut u32, out_pix_slots: *mut u32,
                                   max_tiles: usize) -> c_int;
    pub fn rtx_strerror(err: c_int) -> *const c_char;
    pub fn rtx_last_hip_error() -> c_int;
    pub fn rtxh_scatter_tiles(frame: *mut u8, height: u32, width: u32, packed: *const u8, first_tile: u32,
                              tile_stride: u32, tile_rows: u32) -> c_int;
    pub fn rtxh_camera_new(eye: *const f32, look_at: *const f32, up: *const f32, u: *mut f32, v: *mut f32, w: *mut f32);
    pub fn rtxh_ref_leaf_rank(n_tris: u32, v0v1v2: *const f32, out_rank: *mut u32) -> c_int;
}

/// Error of a library call, with the library's own text.
pub fn check(rc: c_int) -> Result<(), String> {
    if rc == RTX_OK {
        Ok(())
    } else {
        let text = unsafe { CStr::from_ptr(rtx_strerror(rc)) };
        Err(format!("librtx: {} [{}]", text.to_string_lossy(), rc))
    }
}
