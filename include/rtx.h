/*
 * rtx.h — C ABI of librtx.so: the MI355X (gfx950) implementation of the
 * per-pixel tracer hot path of antoinedesbois/Ray-Tracer-Rust.
 *
 * The reference has no FFI or plugin interface.  The seam
 * this library replaces is the body of the thread fan-out in render(),
 * src/main.rs:275-303: everything between "have a Scene and the random-sample
 * table" and "have a filled RGB8 image", i.e. render_pixel() (src/main.rs:180-240)
 * applied to every pixel, with the src/tracer tree underneath.  A Rust caller binds
 * these entry points with an `extern "C"` block.
 *
 * Conventions
 *   - plain pointers and sizes only; every input/output host buffer is owned
 *     by the caller and may be freed as soon as the call returns;
 *   - RtxScene is an opaque library-owned handle; device memory never escapes,
 *     except through the *_device entry point, which writes into a device
 *     buffer the caller owns;
 *   - every function returns RTX_OK (0) or a negative RtxError; nothing throws
 *     or aborts across the boundary (the reference's convention is
 *     unwrap()-panic, src/main.rs:291,297,302,313-315 — not carried over);
 *   - rtx_scene_create/destroy are not re-entrant per handle; rendering on
 *     DISTINCT devices may run concurrently from distinct host threads on one
 *     scene (mirrors one-thread-per-slice, src/main.rs:275-299); same-device
 *     calls are serialised internally;
 *   - there is no CPU fallback: rendering without a usable HIP device fails
 *     with RTX_ERR_NO_DEVICE.
 *
 * Pixel/row conventions follow the reference: px is the column, py the row,
 * byte offset of a pixel in an RGB8 frame = (py*width + px)*3
 * (put_pixel(px,py), src/main.rs:293-294).
 */
#ifndef RTX_H
#define RTX_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RTX_ABI_VERSION 3

typedef enum RtxError {
    RTX_OK              =  0,
    RTX_ERR_BAD_ARG     = -1,  /* null pointer, zero size, row range outside the frame ...        */
    RTX_ERR_NO_DEVICE   = -2,  /* no HIP device / device index out of range                       */
    RTX_ERR_HIP         = -3,  /* a HIP runtime call failed (rtx_last_hip_error() has the code)   */
    RTX_ERR_OOM         = -4,  /* host or device allocation failed                                */
    RTX_ERR_UNSUPPORTED = -5,  /* e.g. non-finite geometry                                        */
    RTX_ERR_INTERNAL    = -6,
    RTX_ERR_IO          = -7   /* host helpers: file not found / parse error                      */
} RtxError;

/* acceleration structure used for closest-hit (results are identical) */
#define RTX_ACCEL_BVH    0u  /* SAH BVH over the triangles' AABBs, wave-uniform traversal (default) */
#define RTX_ACCEL_BRUTE  1u  /* one leaf holding every triangle: brute-force scan                    */

/* The reference's own tree (BoundingVolumeHierarchy::new, bounding_volume_hierarchy.rs:173-226; O(n^2)).
 * It is NOT the traversal structure: for rays whose direction components are all non-zero the
 * result provably does not depend on the tree.  It is needed for two corner
 * cases, which is why the library rebuilds it on the host: exact-distance ties (the right-most leaf
 * wins) and rays with a zero direction component, whose result in the reference depends on the tree
 * (a -0.0 component rejects an ancestor box through +-inf while a flat leaf box accepts through
 * ignored NaNs); wavefronts holding such a ray are traced against the reference tree itself. */
#define RTX_REFTREE_AUTO   0u  /* build it when n_tris <= 50,000 (beyond that the reference cannot run) */
#define RTX_REFTREE_ALWAYS 1u
#define RTX_REFTREE_NEVER  2u  /* ties: tie_rank or index order; zero-component rays: the library's tree */

/*
 * Flat description of the reference's Scene (src/tracer/utils/scene.rs:6-12):
 *   width,height           Scene.width/height
 *   eye,u,v,w,distance     Camera after Camera::new (camera.rs:17-35); rtxh_camera_new computes u,v,w
 *   light_v0..2            vertices of Light.primitives[0] (light.rs:11-13 samples only that one)
 *   v0v1v2, rgb            the Vec<Primitive> handed to BoundingVolumeHierarchy::new, in that order
 *                          (Triangle arm: v0,v1,v2 + Color); the library derives e1, e2, normal
 *                          with Triangle::new's operation order (triangle.rs:22-34)
 *   tie_rank               optional, n_tris entries: position of each triangle in the left-to-right
 *                          leaf order of the reference BVH.  When two triangles are hit at exactly
 *                          the same distance the reference returns the right-most one
 *                          (bounding_volume_hierarchy.rs:123-130); the library returns the one with
 *                          the larger tie_rank.  NULL = taken from the reference tree when the
 *                          library builds it (reference_tree), else the index.  rtxh_ref_leaf_rank
 *                          computes it (restates bounding_volume_hierarchy.rs:173-226).
 *   reference_tree         RTX_REFTREE_*
 *   nb_ray,nb_light_sample NB_RAY / NB_LIGHT_SAMPLE (src/main.rs:38-39)
 *   samples,n_samples      the random-sample table, n_samples pairs (s.0,s.1) interleaved
 *                          (src/main.rs:253,262-265); NB_RAND_SAMPLE = 2,000,000 in the reference
 */
typedef struct RtxSceneDesc {
    uint32_t width, height;
    float eye[3], u[3], v[3], w[3];
    float distance;
    float light_v0[3], light_v1[3], light_v2[3];
    uint32_t n_tris;
    const float *v0v1v2;        /* n_tris x 9 */
    const float *rgb;           /* n_tris x 3 */
    const uint32_t *tie_rank;   /* n_tris, or NULL */
    uint32_t nb_ray, nb_light_sample;
    const float *samples;       /* n_samples x 2 */
    uint32_t n_samples;
    uint32_t accel;             /* RTX_ACCEL_* */
    uint32_t leaf_max;          /* max triangles per BVH leaf; 0 = library default */
    uint32_t reference_tree;    /* RTX_REFTREE_* */
    /* Sphere arm of Primitive (src/tracer/primitives/sphere.rs:12-29); n_spheres = 0 for the reference's main() */
    uint32_t n_spheres;
    const float *spheres;       /* n_spheres x 4: origin x,y,z, radius */
    const float *sphere_rgb;    /* n_spheres x 3 */
    const uint8_t *kinds;       /* order of the Vec<Primitive>: n_tris + n_spheres bytes, 0 = next triangle,
                                   1 = next sphere; NULL = all triangles, then all spheres.  Primitive indices
                                   (tie_rank entries, statistics) are positions in that Vec. */
} RtxSceneDesc;

typedef struct RtxStats {
    uint64_t primary_rays;      /* pixels rendered x nb_ray                                     */
    uint64_t primary_hits;      /* primary rays with a closest hit                              */
    uint64_t shadow_rays;       /* nb_light_sample x primary_hits                               */
    uint64_t rays;              /* R_total = primary_rays + shadow_rays                         */
    uint64_t box_tests;         /* ray-box slab tests executed (per lane)                       */
    uint64_t tri_tests;         /* ray-triangle Möller–Trumbore tests executed (per lane)       */
    uint64_t wave_node_visits;  /* BVH node records fetched (per wave)                          */
    uint64_t wave_tri_visits;   /* triangle records fetched (per wave)                          */
    uint64_t redo_tiles;        /* 8x8 tiles re-rendered with the literal reference traversal   */
    double   kernel_ms;         /* hipEvent time of the kernel(s) of this call                  */
    double   total_ms;          /* host wall time of the call (launch + D2H + gather)           */
} RtxStats;

typedef struct RtxSceneInfo {
    uint32_t n_tris, n_nodes, n_leaves, max_leaf_tris, depth;
    uint32_t n_light_points;
    uint32_t n_ref_nodes;       /* records of the reference-tree stream (0 = not built) */
    uint32_t n_global;      /* triangles as large as the scene (the ground): tested by every walk up front, outside the tree */
    uint64_t node_bytes, tri_bytes, shade_bytes, sample_bytes;
} RtxSceneInfo;

typedef struct RtxScene RtxScene;

/* ---- device path --------------------------------------------------------- */

int rtx_abi_version(void);
/* number of usable HIP devices (0 when there is none; never negative) */
int rtx_device_count(void);

/* Host-side preparation only (no device is touched): copies the inputs, derives e1/e2/normal,
 * the 100 light points, the gamma threshold table and the acceleration structure. */
int rtx_scene_create(const RtxSceneDesc *desc, RtxScene **out);
void rtx_scene_destroy(RtxScene *scene);
int rtx_scene_info(const RtxScene *scene, RtxSceneInfo *info);

/* Upload the prepared scene to `device` (idempotent; rendering does it on first use). */
int rtx_scene_upload(RtxScene *scene, int device);

/* Render rows [row0,row0+nrows) on `device` into out_rgb (nrows*width*3 bytes, host).
 * stats may be NULL; when non-NULL the launch also counts tests (slightly slower).
 * One launch (this call, or one device's share of rtx_render_frame / rtx_render_tiles_device) covers at most
 * 2^25 tiles of 8x8 pixels (2^31 pixels); beyond that the call fails with RTX_ERR_HIP: render in bands. */
int rtx_render_rows(RtxScene *scene, int device, uint32_t row0, uint32_t nrows,
                    uint8_t *out_rgb, RtxStats *stats);

/* Whole frame, row tiles of `tile_rows` rows dealt round-robin to devices[0..n_devices)
 * (tile t -> devices[t % n_devices]); out_rgb is height*width*3 bytes, host.  A device may be named more than
 * once: its shares are rendered one after another (how the multi-share path is rehearsed on one GPU).  Device locks
 * are taken in ascending device order whatever the order of the array; on an error the launches and copies already
 * in flight are waited for before the call returns. */
int rtx_render_frame(RtxScene *scene, const int *devices, int n_devices, uint32_t tile_rows,
                     uint8_t *out_rgb, RtxStats *stats);

/* Device-resident variant for callers that own device memory and a stream (one process per GPU):
 * renders row tiles first_tile, first_tile+tile_stride, ... (tile t = rows [t*tile_rows,
 * (t+1)*tile_rows) clipped to the frame) and packs them one after another into d_out_rgb
 * (device pointer, d_out_bytes >= rtx_tiles_bytes(...)).  The launch is asynchronous on
 * `stream` (a hipStream_t; NULL = the default stream); inputs must already be uploaded or are
 * uploaded synchronously first.  d_counters: NULL, or a device buffer of 8 uint64 that the kernel
 * ADDS its counters to (primary_hits, box_tests, tri_tests, wave_node_visits, wave_tri_visits, redo_tiles).
 * Launches on one device must be ordered on one stream (the library keeps a per-device work queue).
 * Each call must be ENQUEUED by the library: do not capture a render launch into a graph and replay it, and do not
 * re-enqueue recorded dispatches.  A launch's kernels take, as arguments, which of two sets of counting words this
 * launch works on — the launch before it zeroed them — and the library advances that choice per call; a replay would run
 * on words nobody zeroed.  (This holds for every entry point that goes through the render pipeline: rtx_render_rows,
 * rtx_render_frame, rtx_render_tiles_device, rtx_render_view_rows and rtx_render_view_rows_device.) */
int rtx_render_tiles_device(RtxScene *scene, int device, uint32_t first_tile, uint32_t tile_stride,
                            uint32_t tile_rows, void *d_out_rgb, size_t d_out_bytes,
                            void *stream, uint64_t *d_counters);
/* rows / bytes the call above produces; rtxh_scatter_tiles puts such a packed share back into a frame */
uint32_t rtx_tiles_rows(const RtxScene *scene, uint32_t first_tile, uint32_t tile_stride, uint32_t tile_rows);
size_t   rtx_tiles_bytes(const RtxScene *scene, uint32_t first_tile, uint32_t tile_stride, uint32_t tile_rows);

/* ---- ray queries: rays the caller supplies ---------------------------------- */
/* The reference's public traversal surface is BoundingVolumeHierarchy::intersect(&Ray) -> Option<HitInfo>
 * (bounding_volume_hierarchy.rs:50-75,228), which render_pixel calls twice (main.rs:187,204).  These entry points are
 * that call for a batch of rays — a bounce, a pick ray, an ambient-occlusion pass, a visibility test between two
 * points — with the reference's semantics bit for bit.  They have kernels of their own and leave the render pipeline
 * and its workspace alone.
 *
 * Outside the parity contract (the calls still terminate and return RTX_OK; the values are unspecified): rays with a
 * non-finite origin or direction, a zero-length direction, or a hit whose t is not finite.  Finite origins may lie
 * anywhere, far outside the scene included: a 64-ray group holding an origin with a coordinate beyond the scene's and
 * the eye's largest walks with the exact box test (slower, same results). */
#define RTX_NO_HIT 0xFFFFFFFFu
typedef struct RtxRayHit {      /* 32 bytes */
    uint32_t prim;              /* position in the Vec<Primitive>, RTX_NO_HIT = None                          */
    float    t;                 /* the distance the leaf rule compared (bvh.rs:64-67): triangle.rs's t, sphere.rs's distance */
    float    p_hit[3];          /* ray.origin + t * ray.direction (bvh.rs:69)                                  */
    float    normal[3];         /* p.get_normal(p_hit): the triangle's unit normal / normalize(p_hit - origin) */
} RtxRayHit;                    /* a miss writes prim = RTX_NO_HIT and zeros                                   */

/* The walk is wave-uniform: a wavefront visits the union of its 64 rays' nodes, so by default a batch of at least a few
 * thousand rays (DESIGN.md "Ray queries") is regrouped on the device first — sorted by direction class, direction octant
 * and a Morton code of the origin — and traced in that order.  Results are written to the rays' own numbers and are the
 * same bytes either way. */
#define RTX_RAYS_KEEP_ORDER    1u  /* trace the rays in the caller's order: no regrouping pass                     */
#define RTX_RAYS_FORCE_REGROUP 2u  /* DIAGNOSTIC: regroup whatever the batch size — how tools/trace_rays_timing.py and the
                                      tests reach the regrouping pass with small batches; no result depends on it      */

/* bvh.intersect(&Ray::new(origin, direction)) per ray: the minimum accepted t; hits with t < 1.0 are ignored
 * (bvh.rs:64-67); on an exact tie the right-most leaf of the reference tree wins (tie_rank).  Colour is not returned:
 * the caller indexes its own rgb with prim.  origins, directions: n_rays x 3 floats, host; a direction may have any
 * length (Ray::new normalises).  NULL pointer, unknown flag or n_rays > 2^28: RTX_ERR_BAD_ARG; n_rays == 0: RTX_OK,
 * no output written; no usable device: RTX_ERR_NO_DEVICE (there is no CPU fallback).
 * stats may be NULL; when non-NULL the counted kernel form runs (same results) and the fields mean:
 *   primary_rays = rays = n_rays, primary_hits = rays with a hit (rtx_occluded_rays: occluded rays), shadow_rays = 0,
 *   box_tests / tri_tests / wave_node_visits / wave_tri_visits as for rendering,
 *   redo_tiles = 64-RAY GROUPS traced with the literal reference traversal because one of their rays has a -0.0, NaN
 *                or infinite direction component,
 *   kernel_ms = device time of the call's kernels (regrouping included), total_ms = host wall time of the call. */
int rtx_trace_rays(RtxScene *scene, int device, uint32_t n_rays, const float *origins, const float *directions,
                   uint32_t flags, RtxRayHit *out_hits, RtxStats *stats);
/* The decision of main.rs:201-231 per ray: the ray is Ray::new(origin, target - origin), D = distance(target, origin);
 * it is occluded iff a closest hit exists and !(distance(origin, p_hit) > D).  out_occluded: n_rays bytes, 1 = occluded,
 * 0 = lit.  Arguments, errors and stats as rtx_trace_rays. */
int rtx_occluded_rays(RtxScene *scene, int device, uint32_t n_rays, const float *origins, const float *targets,
                      uint32_t flags, uint8_t *out_occluded, RtxStats *stats);
/* Device-resident variants, asynchronous on `stream` (a hipStream_t; NULL = the default stream), as
 * rtx_render_tiles_device is: inputs and outputs are device pointers the caller owns (floats 4-byte aligned, d_hits
 * 16-byte aligned: else RTX_ERR_BAD_ARG); the regrouping pass runs on the same stream in library-owned buffers, so
 * device-resident query launches on one device must be ordered on one stream.  The host entry points above use the
 * same buffers on the library's own stream; they wait (on the device, by an event) for the most recent device-resident
 * query launch first, so they may be mixed with these freely. */
int rtx_trace_rays_device(RtxScene *scene, int device, uint32_t n_rays, const void *d_origins, const void *d_directions,
                          uint32_t flags, void *d_hits, void *stream);
int rtx_occluded_rays_device(RtxScene *scene, int device, uint32_t n_rays, const void *d_origins, const void *d_targets,
                             uint32_t flags, void *d_occluded, void *stream);

/* ---- shading rays the caller supplies ---------------------------------------- */
/* render_pixel's body (main.rs:182-239) for a batch: per ray the closest hit, nb_light_sample shadow rays towards the
 * scene's area light, the sequential f32 sum and Color::to_rgba — the colour the reference gives a pixel whose rays
 * create_rays did not make: another camera model, a crop, a second bounce, a light-map bake, a picker.  Kernels of its
 * own, beside the render pipeline and the ray queries.
 *
 * A "pixel" is nb_ray consecutive rays of the arrays (nb_ray is the scene's; the reference's value is 1): origins and
 * directions hold n_pixels * nb_ray x 3 floats, host; a direction may have any length (Ray::new normalises).  Pixel p
 * gets exactly what render_pixel computes when create_rays returns Ray::new(origins[p*nb_ray + r], directions[p*nb_ray
 * + r]) for r = 0..nb_ray.  Each ray with a closest hit runs i = 0..nb_light_sample: the light point is the scene's
 * light_points[r][i] (table entry (r*nb_ray + i) % n_samples, rtx_scene_light_points), the shadow ray is
 * Ray::new(p_hit, p - p_hit), lnd = |normal . direction|, the decision is that of main.rs:218-232 (rtx_occluded_rays'),
 * and avg += (colour * lnd) / (nb_ray * nb_light_sample) as f32, channel by channel in that order; an occluded sample
 * adds nothing (the reference adds black / denom = +0.0), as in the render pipeline.  A pixel whose rays all miss is
 * {0,0,0}, bytes 0,0,0, hits = 0.  Results do not depend on the tracing order: with or without the regrouping pass
 * (the key is built from each pixel's ray 0) a pixel's 16 bytes are the same.
 * Outside the parity contract, as for the ray queries: non-finite inputs, zero-length directions, non-finite t (the call
 * still terminates with RTX_OK). */
typedef struct RtxPixelShade {   /* 16 bytes, one 16-byte store */
    float   linear[3];           /* render_pixel's avg_col (main.rs:182-239) for this pixel's rays */
    uint8_t rgb8[3];             /* Color::to_rgba of it: the scene's gamma thresholds, as the frame's bytes */
    uint8_t hits;                /* how many of the pixel's nb_ray rays had a closest hit, saturating at 255 */
} RtxPixelShade;
/* out_shade: n_pixels records.  out_hits: NULL, or n_pixels * nb_ray records, byte-identical to what rtx_trace_rays
 * writes for the same rays.  flags: RTX_RAYS_KEEP_ORDER, RTX_RAYS_FORCE_REGROUP (the regrouping threshold counts
 * pixels).  NULL scene / origins / directions / out_shade, unknown flag or n_pixels * nb_ray > 2^28: RTX_ERR_BAD_ARG;
 * n_pixels == 0: RTX_OK, nothing written; no usable device: RTX_ERR_NO_DEVICE (there is no CPU fallback).
 * stats may be NULL; when non-NULL the counted kernel form runs (same results) and the fields mean:
 *   primary_rays = n_pixels * nb_ray, primary_hits = rays with a closest hit, shadow_rays = nb_light_sample *
 *   primary_hits, rays = primary_rays + shadow_rays, box_tests / tri_tests / wave_node_visits / wave_tri_visits as for
 *   rendering, redo_tiles = 64-LANE WALKS, primary or shadow, that took the literal reference traversal (a -0.0, NaN or
 *   infinite direction component among their rays), kernel_ms / total_ms as rtx_trace_rays. */
int rtx_shade_rays(RtxScene *scene, int device, uint32_t n_pixels, const float *origins, const float *directions,
                   uint32_t flags, RtxPixelShade *out_shade, RtxRayHit *out_hits /* may be NULL */, RtxStats *stats);
/* Device-resident variant, asynchronous on `stream`, as rtx_trace_rays_device is: device pointers the caller owns
 * (floats 4-byte aligned; d_shade and, when given, d_hits 16-byte aligned: else RTX_ERR_BAD_ARG).  It uses the ray
 * queries' regrouping buffers, so the same rule holds across all of them: device-resident query and shade launches on
 * one device must be ordered on one stream, and the host entry points wait (by an event) for the most recent of them. */
int rtx_shade_rays_device(RtxScene *scene, int device, uint32_t n_pixels, const void *d_origins, const void *d_directions,
                          uint32_t flags, void *d_shade, void *d_hits /* may be NULL */, void *stream);

/* ---- any pinhole view of the uploaded scene ----------------------------------- */
/* rtx_render_rows renders the camera rtx_scene_create was given.  These entry points render a rectangle of ANY view —
 * another eye, another frame, a crop, a thumbnail — of the scene as it is uploaded: no new scene, no tree build, no ray
 * arrays.  Pixel (px, py) gets exactly render_pixel(px, py) (main.rs:180-240) of a reference Scene that has the view's
 * width, height and camera; primitives, light, nb_ray, nb_light_sample and the sample table are the uploaded scene's.
 * The rays are create_rays' (main.rs:151-178) bit for bit.  Kernels of its own, beside the render pipeline, the ray
 * queries and ray shading: one wavefront per 8x8 tile of the rectangle, no regrouping pass. */
typedef struct RtxView {          /* 76 bytes, alignment 4 */
    uint32_t width, height;       /* the frame create_rays sees: w, h of main.rs:156-157 and the table index
                                     (px*width + py + i) % n_samples (u32 arithmetic) */
    float eye[3], u[3], v[3], w[3];
    float distance;               /* Camera after Camera::new (camera.rs:17-35); rtxh_camera_new computes u, v, w */
    uint32_t x0, y0, nx, ny;      /* the pixels to render: columns [x0,x0+nx) x rows [y0,y0+ny) */
} RtxView;

/* the scene's own camera and whole frame: what rtx_scene_create was given */
int rtx_scene_view(const RtxScene *scene, RtxView *out);
/* out_rgb:   NULL or ny*nx*3 bytes, rows packed: pixel (x,y) at ((y-y0)*nx + (x-x0))*3 — the bytes rtx_render_rows of a
 *            scene created with that camera holds for the pixel;
 * out_shade: NULL or ny*nx records, same order; out_hits: NULL or ny*nx*nb_ray records, a pixel's rays consecutive — both
 *            byte-identical to what rtx_shade_rays / rtx_trace_rays return for the view's rays.
 * RTX_ERR_BAD_ARG: NULL scene or view, all three outputs NULL, width == 0 or height == 0, width*height >= 2^31, a
 * rectangle outside the frame, nx*ny*nb_ray > 2^28.  nx == 0 or ny == 0: RTX_OK, nothing written, stats zeroed, no device
 * needed.  No usable device: RTX_ERR_NO_DEVICE (there is no CPU fallback).  Non-finite camera values are outside the
 * parity contract (the call still terminates with RTX_OK).  The eye may lie anywhere: beyond the scene's and its own
 * camera's largest coordinate the primary walks use the exact box test (slower, same results).
 * stats may be NULL; when non-NULL the counted kernel form runs (same results) and the fields mean what rtx_shade_rays
 * gives them, with primary_rays = nx*ny*nb_ray.
 * A view call leaves every later render, query or shade call on the scene unchanged. */
int rtx_render_view(RtxScene *scene, int device, const RtxView *view, uint8_t *out_rgb, RtxPixelShade *out_shade,
                    RtxRayHit *out_hits, RtxStats *stats);
/* Device-resident variant, asynchronous on `stream` (a hipStream_t; NULL = the default stream): device pointers the caller
 * owns, each NULL or sized as above (d_shade and d_hits 16-byte aligned: else RTX_ERR_BAD_ARG).  It uses no library
 * buffer: no ordering rule ties it to the query or shade calls.  The scene is uploaded (synchronously) first if needed. */
int rtx_render_view_device(RtxScene *scene, int device, const RtxView *view, void *d_rgb, void *d_shade, void *d_hits,
                           void *stream);

/* ---- any view through the render pipeline --------------------------------------- */
/* Rows [y0, y0+ny) of the view's frame through the RENDER PIPELINE (scheduling pass + shading pass: per-tile cuts, compacted
 * hit records, the cost-ordered schedule — what rtx_render_rows runs), full width: x0 == 0 and nx == width, else
 * RTX_ERR_BAD_ARG.  out_rgb: ny*width*3 bytes, rows packed — the bytes rtx_render_view gives for the same view, i.e.
 * rtx_render_rows(y0, ny) of a scene created with that camera.  A turntable is one scene and N of these calls.
 *
 * The pipeline's kernels read the camera and the frame from their argument block, which is built per launch; what a new
 * eye needs made is the stream its primary rays walk (of every node's children the one nearer the EYE first: an ordering
 * for speed, no result depends on it).  The library keeps ONE such stream per device in a buffer of its own and makes it on
 * the device (two small kernels, rtx_aim.hip) on the call's stream, ahead of the scheduling pass.  Cache rule: the buffer
 * remembers the 12 bytes of the eye it was aimed at and the stream it was aimed on; a call with the same eye bytes on the
 * same stream runs no aim kernel, any other call runs them again.  A scene without a primary stream of its own
 * (RTX_ACCEL_BRUTE, or nothing beside the global triangles) aims nothing: its primary rays walk rtx_scene_nodes' stream.
 *
 * Errors: RTX_ERR_BAD_ARG for rtx_render_view's argument checks (NULL scene / view / output, width == 0 or height == 0,
 * width*height >= 2^31, rows outside the frame) and for a rectangle that is not the full width; the device variant also for
 * d_bytes < ny*width*3.  ny == 0: RTX_OK, nothing written, stats zeroed, no device needed.
 * Range rule: RTX_ERR_UNSUPPORTED unless max |eye[k]| <= cull_delta * 2^19 — the largest coordinate magnitude of the scene's
 * primitives and the eye rtx_scene_create was given (a NaN fails the comparison); checked before a device is looked for.
 * The pipeline's walks use the multiply-based box test only, whose culling planes were moved outwards for origins within
 * that magnitude: the pipeline has no exact-slab form to fall back on, and the tile shaft test's margin was sized without
 * such an eye.  rtx_render_view serves those eyes (its primary walks switch to the exact box test), as it serves rectangles
 * narrower than the frame and shade / hit records.  No usable device: RTX_ERR_NO_DEVICE (there is no CPU fallback).
 * stats mean what they mean for rtx_render_rows, with primary_rays = ny*width*nb_ray and redo_tiles in tiles; kernel_ms
 * includes the aim kernels when they run.  The launches count in rtx_launch_timings (the aim kernels lie outside both of its
 * passes) and rtx_debug_tile_descs like any render launch, and the rule of rtx_render_tiles_device holds unchanged:
 * pipeline launches on one device — these included — must be ordered on one stream, and none may be captured and replayed.
 * A view call leaves every later render, query, shade or view call on the scene unchanged: the prepared scene and its
 * uploaded streams are not written. */
int rtx_render_view_rows(RtxScene *scene, int device, const RtxView *view, uint8_t *out_rgb, RtxStats *stats);
/* Device-resident variant, asynchronous on `stream` (a hipStream_t; NULL = the default stream), as rtx_render_tiles_device
 * is: d_rgb is a device pointer the caller owns, d_bytes >= ny*width*3; d_counters: NULL or rtx_render_tiles_device's 8
 * uint64 the kernels ADD to.  The scene is uploaded (synchronously) first if needed. */
int rtx_render_view_rows_device(RtxScene *scene, int device, const RtxView *view, void *d_rgb, size_t d_bytes,
                                void *stream, uint64_t *d_counters);
/* Diagnostic: runs the aim kernels for `eye` on `device` (whatever the buffer holds), blocks, and copies the device's aimed
 * stream back: n_nodes*8 dwords in NodeRec word order, as rtx_scene_nodes.  A scene without a primary stream of its own:
 * its uploaded stream, nothing run. */
int rtx_debug_aimed_nodes(RtxScene *scene, int device, const float eye[3], uint32_t *out_dwords);

/* ---- another light for views and shaded rays ------------------------------------- */
/* rtx_scene_create turns the light into nb_ray * nb_light_sample light points once.  These entry points shade with ANY
 * area light of the reference's kind and any sample count, on the scene as it is uploaded: no new scene, no tree build, no
 * upload.  A pixel is render_pixel's (main.rs:180-240) of a reference Scene that differs in two ways: scene.light.primitives[0]
 * is the given triangle, and NB_LIGHT_SAMPLE is the given count — the shadow loop's bound (main.rs:193) and the denominator
 * nb_ray * nb_light_sample (main.rs:211).  Light point [r][i] is get_sample(T[(r*nb_ray + i) % n_samples]) (main.rs:194-196,
 * triangle.rs:113-127; the third weight is v * sqrt(u), as the reference has it).
 *
 * The library makes the points on the device (one small kernel, rtx_light.hip) on the call's stream, ahead of the view or
 * shade kernel, in ONE buffer of its own per device, which grows only (growing waits for the device).  There is no cache:
 * every lit call runs the kernel.  The ordering rule is the regrouping buffers': device-resident lit launches on one device
 * must be ordered on one stream; the host entry points use the same buffer on the library's stream and wait (on the device,
 * by an event) for the most recent device-resident lit launch first, so they may be mixed with those freely.
 * rtx_shade_rays_lit* also uses the regrouping buffers and inherits their rule unchanged (rtx_shade_rays_device).
 *
 * There is no range rule on the light: a vertex may lie anywhere, beyond the scene's largest coordinate included.  A shadow
 * ray's ORIGIN is the hit point, which is what the walks' choice of box test is voted on; the light point is the ray's
 * target, unrestricted as rtx_occluded_rays' targets are.
 * The render pipeline reads more of the light than its points — the tour, the boxes and the shaft margin that
 * rtx_scene_create makes: its lit form is rtx_render_view_rows_lit, below, which makes them per call.
 * A lit call leaves every later call on the scene unchanged: the prepared scene and its uploaded light are not written. */
typedef struct RtxLight {          /* 40 bytes, alignment 4 */
    float v0[3], v1[3], v2[3];     /* Light.primitives[0] (light.rs:11-13): the triangle get_sample samples */
    uint32_t nb_light_sample;      /* NB_LIGHT_SAMPLE for this call (main.rs:39); 0 = the scene's */
} RtxLight;

/* the light and the sample count rtx_scene_create was given */
int rtx_scene_light(const RtxScene *scene, RtxLight *out);
/* Each lit call is its unlit twin — rtx_render_view, rtx_render_view_device, rtx_shade_rays, rtx_shade_rays_device — in
 * every respect: argument checks, outputs, flags, regrouping, alignment rules.  Beyond those:
 *   RTX_ERR_BAD_ARG      light == NULL, or nb_ray * count > 2^20 (count: the light's, or the scene's for 0);
 *   nx == 0, ny == 0 or n_pixels == 0: RTX_OK as in the twin, nothing written, stats zeroed, no device needed;
 *   RTX_ERR_UNSUPPORTED  a vertex coordinate that is not finite — decided on the host, before a device is looked for.
 * The light is read before the call returns.  stats: as the twin's, with shadow_rays = count * primary_hits; kernel_ms
 * includes the light kernel. */
int rtx_render_view_lit(RtxScene *scene, int device, const RtxView *view, const RtxLight *light, uint8_t *out_rgb,
                        RtxPixelShade *out_shade, RtxRayHit *out_hits, RtxStats *stats);
int rtx_render_view_lit_device(RtxScene *scene, int device, const RtxView *view, const RtxLight *light, void *d_rgb,
                               void *d_shade, void *d_hits, void *stream);
int rtx_shade_rays_lit(RtxScene *scene, int device, uint32_t n_pixels, const float *origins, const float *directions,
                       uint32_t flags, const RtxLight *light, RtxPixelShade *out_shade, RtxRayHit *out_hits /* may be NULL */,
                       RtxStats *stats);
int rtx_shade_rays_lit_device(RtxScene *scene, int device, uint32_t n_pixels, const void *d_origins, const void *d_directions,
                              uint32_t flags, const RtxLight *light, void *d_shade, void *d_hits /* may be NULL */,
                              void *stream);
/* Diagnostic: runs the light kernel for `light` on `device`, blocks, and copies the device's points back: nb_ray * count
 * x 3 floats, as rtx_scene_light_points_for.  Errors as the lit calls'. */
int rtx_debug_light_points(RtxScene *scene, int device, const RtxLight *light, float *out);

/* ---- another light through the render pipeline ------------------------------------ */
/* rtx_render_view_rows under ANY light: the bytes are rtx_render_rows(y0, ny) of a reference Scene created with the view's
 * camera and frame, the given triangle as light.primitives[0] and the given count as NB_LIGHT_SAMPLE — the bytes
 * rtx_render_view_lit gives for the same view and light, at the pipeline's speed.
 *
 * The pipeline's kernels are the ones rtx_render_view_rows launches, unchanged; they read the light as five fields of their
 * argument block, which a lit call swaps: the points (rtx_light.hip's kernel), the order each batch of 128 samples is
 * walked in and the points' box per primary ray (two kernels, rtx_tour.hip), the sample count, and the tile shaft test's
 * margin, which the host computes (O(nb_ray * count), microseconds) as rtx_scene_create does: 2^-16 x the largest coordinate
 * magnitude of the scene, the eye rtx_scene_create was given and this light's points, + 2^-100.  The light kernels run on
 * the call's stream behind the aim kernels, ahead of the scheduling pass, in buffers of the library's own per device
 * beside the points', under the same rules: they grow only (growing waits for the device), there is no cache (every lit
 * call runs the kernels), device-resident lit launches on one device must be ordered on one stream, and the host entry
 * points wait (on the device, by an event) for the most recent of them.  The tour is a statement of its own
 * (rtx_scene_light_walk_for): rtx_scene_create's scan with f32 distances, so that the device makes it word for word; it
 * decides the order shadow rays are walked in, never a byte.
 *
 * Each call is its unlit twin — rtx_render_view_rows, rtx_render_view_rows_device — in every other respect: full width only,
 * the eye's range rule (RTX_ERR_UNSUPPORTED before a device is looked for), ny == 0 gives RTX_OK with stats zeroed and no
 * device needed, d_bytes is checked, stats as rtx_render_rows' with shadow_rays = count * primary_hits, kernel_ms includes the
 * aim and light kernels, the launch counts in rtx_launch_timings (the light kernels lie outside both passes, as the aim
 * kernels do) and rtx_debug_tile_descs, no capture and replay, pipeline launches on one device ordered on one stream.
 * The lit calls' own rules: RTX_ERR_BAD_ARG for light == NULL or nb_ray * count > 2^20 (count: the light's, or the scene's
 * for 0); RTX_ERR_UNSUPPORTED for a vertex coordinate that is not finite, decided on the host; the light is read before the
 * call returns.  One more rule, rtx_scene_create's own: RTX_ERR_UNSUPPORTED when the margin above is not finite — a pipeline
 * call accepts exactly the lights rtx_scene_create would accept.  There is no other range rule on the light: it is never a
 * ray's origin, and the margin grows with its coordinates as it does for a created scene.  When the scene's own count is 0
 * and the light's is 0 no light kernel runs: the bytes are the unlit call's.
 * A lit call leaves every later call on the scene unchanged. */
int rtx_render_view_rows_lit(RtxScene *scene, int device, const RtxView *view, const RtxLight *light, uint8_t *out_rgb,
                             RtxStats *stats);
int rtx_render_view_rows_lit_device(RtxScene *scene, int device, const RtxView *view, const RtxLight *light, void *d_rgb,
                                    size_t d_bytes, void *stream, uint64_t *d_counters);
/* Diagnostic: runs the light kernels for `light` on `device`, blocks, and copies back the tour records — nb_ray * count x 4
 * words: x, y, z and, as bits, the sample's index within its batch, in walk order — and the boxes, nb_ray x 6 floats (lo
 * xyz, hi xyz).  Errors as the lit calls' (the margin is not looked at); both outputs are required. */
int rtx_debug_light_walk(RtxScene *scene, int device, const RtxLight *light, float *out_tour, float *out_boxes);

/* ---- posing an uploaded scene's triangles ----------------------------------------- */
/* Geometry that moves without a new scene, a tree build or an upload.  A pose is n_tris x 9 floats in the layout of
 * RtxSceneDesc.v0v1v2: one entry per triangle of the Vec<Primitive>, in Vec order with spheres skipped.  Spheres and
 * colours stay as uploaded (rtx_scene_pose_prims, below, poses them too), and the triangle count does not change.
 *
 * What a pose makes, on the device, on the call's stream, in buffers of the library's own (grow-only; growing waits for
 * the device; ONE pose per scene per device: a new pose replaces the previous one; the uploaded scene is never written):
 *   primitive record j (leaf order, caller index idx): v0, e1, e2 and the own box from the posed triangle by Triangle::new
 *     and get_bounding_box (triangle.rs:22-56) — the one text rtx_scene_create runs on the host — idx unchanged; a sphere's
 *     record is copied;
 *   shading record idx: the normal from the posed triangle (a zero-area triangle: NaN, bits unspecified), rgb and kind
 *     unchanged, the tie rank by the rule below; a sphere's record is copied, rank aside;
 *   node record i: the tree keeps its shape (link and info unchanged).  Every record of the stream covers a contiguous run
 *     [first_i, first_i + count_i) of the primitive array; its posed box is the fminf / fmaxf fold of those records' own
 *     boxes, each plane then moved outwards by the SCENE's cull_delta in f32 (the sign of a zero is lost in the move: any
 *     fold order gives the same words).  The two tables this needs — (first, count) per node, Vec position -> triangle
 *     number — are made on the host once per scene and uploaded with the first pose.
 * rtx_scene_posed_records is the host statement of these words; rtx_debug_pose reads the device's back.
 *
 * Range rule: every posed coordinate must be finite and of magnitude at most M, the largest coordinate magnitude of the
 * created scene's primitives and eye (rtx_scene_pose_bound; 10,000 for main()'s scenes: the ground) — the bound
 * cull_delta and the ray-batch calls' origin bound were sized for.  rtx_scene_pose decides it on the host, before a
 * device is looked for: RTX_ERR_UNSUPPORTED.  For rtx_scene_pose_device it is a stated precondition: outside it the calls
 * still terminate (the topology is fixed) and the values are unspecified.
 *
 * Parity: a posed call returns what the same call returns on a reference Scene holding the posed vertices, everything
 * else the uploaded scene's.  For rays without a zero direction component results do not depend on the tree, so the
 * refitted tree gives the reference's answer for the posed primitives.  Ties and 64-ray groups with a hard direction (a
 * component -0.0, NaN or infinite) follow reference_tree:
 *   RTX_REFTREE_NEVER (rtx_scene_pose_device always): ties by tie_rank (per Vec position, as RtxSceneDesc.tie_rank), or
 *     by index when it is NULL; hard groups walk the refitted stream with the reference's box test — the result of SOME
 *     tree over these primitives, RTX_REFTREE_NEVER's existing rule;
 *   RTX_REFTREE_ALWAYS, or RTX_REFTREE_AUTO by rtx_scene_create's rule (rtx_scene_pose only): the reference's own tree
 *     for the posed primitives is built on the host (O(n^2)) and uploaded beside the pose: it gives the ranks (unless
 *     tie_rank is given) and the stream hard groups walk.
 *
 * rtx_scene_pose: RTX_ERR_BAD_ARG for a NULL scene or v0v1v2 or an unknown reference_tree; stats (may be NULL): kernel_ms
 * is the pose kernels' time, the counters are zero.  Blocks until the pose stands.
 * rtx_scene_pose_device: the caller's device arrays (4-byte aligned; d_tie_rank may be NULL) on the caller's stream,
 * nothing waited for; they must stay valid until the kernels have run.
 * Ordering is the lit buffers': device-resident poses and posed launches on one device must be ordered on one stream, and
 * the host entry points wait (on the device, by an event) for the most recent of them. */
int rtx_scene_pose_bound(const RtxScene *scene, float *out_magnitude);
int rtx_scene_pose(RtxScene *scene, int device, const float *v0v1v2, const uint32_t *tie_rank /* may be NULL */,
                   uint32_t reference_tree, RtxStats *stats);
int rtx_scene_pose_device(RtxScene *scene, int device, const void *d_v0v1v2, const void *d_tie_rank /* may be NULL */,
                          void *stream);
/* Each posed call is its unposed twin — rtx_trace_rays, rtx_occluded_rays, rtx_shade_rays, rtx_render_view and their
 * _device forms — in every respect (argument checks, outputs, flags, regrouping, alignment, stats), and launches the
 * kernels its twin launches, with the geometry pointers of its argument block swapped for the pose's.  light: NULL for the
 * scene's light, else the call is its _lit twin.  RTX_ERR_BAD_ARG when `device` holds no pose of this scene.  A posed call
 * leaves every later unposed call unchanged.  The render pipeline's posed form is rtx_render_view_rows_posed, below. */
int rtx_trace_rays_posed(RtxScene *scene, int device, uint32_t n_rays, const float *origins, const float *directions,
                         uint32_t flags, RtxRayHit *out_hits, RtxStats *stats);
int rtx_occluded_rays_posed(RtxScene *scene, int device, uint32_t n_rays, const float *origins, const float *targets,
                            uint32_t flags, uint8_t *out_occluded, RtxStats *stats);
int rtx_trace_rays_posed_device(RtxScene *scene, int device, uint32_t n_rays, const void *d_origins, const void *d_directions,
                                uint32_t flags, void *d_hits, void *stream);
int rtx_occluded_rays_posed_device(RtxScene *scene, int device, uint32_t n_rays, const void *d_origins, const void *d_targets,
                                   uint32_t flags, void *d_occluded, void *stream);
int rtx_shade_rays_posed(RtxScene *scene, int device, uint32_t n_pixels, const float *origins, const float *directions,
                         uint32_t flags, const RtxLight *light /* NULL = the scene's */, RtxPixelShade *out_shade,
                         RtxRayHit *out_hits /* may be NULL */, RtxStats *stats);
int rtx_shade_rays_posed_device(RtxScene *scene, int device, uint32_t n_pixels, const void *d_origins, const void *d_directions,
                                uint32_t flags, const RtxLight *light /* NULL = the scene's */, void *d_shade,
                                void *d_hits /* may be NULL */, void *stream);
int rtx_render_view_posed(RtxScene *scene, int device, const RtxView *view, const RtxLight *light /* NULL = the scene's */,
                          uint8_t *out_rgb, RtxPixelShade *out_shade, RtxRayHit *out_hits, RtxStats *stats);
int rtx_render_view_posed_device(RtxScene *scene, int device, const RtxView *view, const RtxLight *light /* NULL = the scene's */,
                                 void *d_rgb, void *d_shade, void *d_hits, void *stream);
/* Host only, no device: the words the pose kernels make.  out_tris: n_prims x 16 words (primitive records, leaf order:
 * v0, e1, e2, own box min, own box max, idx); out_shade: n_prims x 8 (normal, rank, rgb, kind; Vec order); out_nodes:
 * n_nodes x 8, NodeRec word order as rtx_scene_nodes, the planes moved by cull_delta.  tie_rank: per Vec position, NULL =
 * the position (RTX_REFTREE_NEVER's rule).  Each output may be NULL.  The vertices are not checked against the range rule. */
int rtx_scene_posed_records(const RtxScene *scene, const float *v0v1v2, const uint32_t *tie_rank, uint32_t *out_tris,
                            uint32_t *out_shade, uint32_t *out_nodes);
/* Diagnostic: blocks and copies the pose `device` holds back, in rtx_scene_posed_records' layout; each output may be NULL.
 * RTX_ERR_BAD_ARG when the device holds no pose. */
int rtx_debug_pose(RtxScene *scene, int device, uint32_t *out_tris, uint32_t *out_shade, uint32_t *out_nodes);

/* The pose through the render pipeline.  Each call is its twin in every respect — rtx_render_view_rows / _device for a NULL
 * light, rtx_render_view_rows_lit / _device otherwise: the argument checks, full width only, the eye's range rule before
 * a device is looked for, ny == 0, d_bytes, stats, rtx_launch_timings, rtx_debug_tile_descs, no capture and replay, the
 * light's rules — and launches the kernels its twin launches.  What differs is what they read: pose_swap's geometry
 * pointers, and the two things the pipeline keeps beside them:
 *   the plane records of the global triangles, made by every pose behind its records (one 16-word record per global
 *     triangle from its posed record: N = e1 x e2 and W = |e1| x |e2| with plus signs in double, N rounded to nearest, W
 *     to the f32 above; K_d = 2^-19 * 2 * (Wx + Wy + Wz) + 2^-100 in double over the rounded W, to the f32 above, or
 *     infinity when a W is not below 2^100) — the words rtx_scene_create makes for the created triangles;
 *   the primary rays' stream, aimed at the view's eye over the pose's refitted stream by rtx_render_view_rows' aim kernels,
 *     in a buffer of the pose's own: it is kept for (eye, stream, pose) and every rtx_scene_pose / rtx_scene_pose_device
 *     takes it away; the unposed calls' aimed stream is neither read nor written, so posed and unposed views of one eye
 *     alternate without aiming either again.  A scene without a primary stream of its own (RTX_ACCEL_BRUTE, or nothing
 *     beside the global triangles) aims nothing: its posed primary rays walk the pose's stream.
 * The margin of the shaft test is the twin's: it is folded from the bound M of the range rule, not from the extent of the
 * geometry.  RTX_ERR_BAD_ARG when `device` holds no pose of this scene.  Ordering: the pose's rule
 * (the host call waits, by an event, for the device-resident poses and posed launches before it; the device-resident one
 * marks the pose busy) and the pipeline's (launches on one device are ordered on one stream).  Parity: the frame of
 * rtx_render_view_rows on a scene created with the posed vertices, byte for byte, under rtx_scene_pose's tie rule. */
int rtx_render_view_rows_posed(RtxScene *scene, int device, const RtxView *view, const RtxLight *light /* NULL = the scene's */,
                               uint8_t *out_rgb, RtxStats *stats);
int rtx_render_view_rows_posed_device(RtxScene *scene, int device, const RtxView *view, const RtxLight *light /* NULL = the scene's */,
                                      void *d_rgb, size_t d_bytes, void *stream, uint64_t *d_counters);
/* Host only, no device: the words a pose makes for the pipeline.  out_planes: n_global x 16 words (v0, N, W, K_d, five
 * zeros, idx: the created scene's plane records, for the posed triangles); out_aimed: n_nodes x 8 words, NodeRec
 * word order: rtx_scene_posed_records' node words (their planes moved by cull_delta once, there) in rtx_scene_aimed_nodes'
 * order for `eye`.  Each output may be NULL; eye may be NULL when out_aimed is.  RTX_ERR_BAD_ARG otherwise for a NULL. */
int rtx_scene_posed_pipeline_records(const RtxScene *scene, const float *v0v1v2, const float eye[3], uint32_t *out_planes,
                                     uint32_t *out_aimed);
/* Diagnostic: the plane records of the pose `device` holds (nothing is written for a scene without global triangles), and
 * the aim kernels run over that pose for `eye` (a scene that aims nothing: the pose's stream), in the layout above;
 * blocks.  Each output may be NULL; eye may be NULL when out_aimed is.  RTX_ERR_BAD_ARG when the device holds no pose. */
int rtx_debug_pose_pipeline(RtxScene *scene, int device, const float eye[3], uint32_t *out_planes, uint32_t *out_aimed);

/* ---- A pose whose tree is rebuilt on the device --------------------------------------------------------------------------
 * rtx_scene_pose_rebuilt / _device are rtx_scene_pose / _device in every respect — the argument checks, the range rule
 * decided on the host before a device is looked for, one pose per scene and device (a new pose of either kind replaces
 * the previous one and takes the pose's aimed stream away), the ordering, stats (kernel_ms: the key kernel, the sort, the
 * record kernel, the refit and the plane kernel) — except the tree: instead of keeping the splits made for the created
 * geometry, the records of the tree proper (every record but the global triangles', which stay records [0, n_global) in
 * their order) are sorted on the device by a 64-bit key, and a balanced tree is laid over the sorted runs.
 *   key: bit 63 the arm (0 triangle, 1 sphere: spheres sort behind all triangles, a leaf never mixes arms); bits 62..0
 *     the 3 x 21-bit Morton interleave (x highest in each triple) of the cells of the centre of the primitive's own posed
 *     box: c = 0.5f * (bmin + bmax), cell = (uint32)((c + M) * S) held to [0, 2^21 - 1], a NaN to cell 0; M is
 *     rtx_scene_pose_bound's, S = 2^21 / (2 M) rounded to f32 once.  A sphere's key comes from its uploaded record
 *     (rtx_scene_pose_prims: from its posed one).
 *   sort: stable — equal keys keep uploaded order.
 *   shape: pre-order, skip-linked, as rtx_scene_nodes: with global triangles and a tree proper, record 0 is the root and
 *     record 1 the global leaf; the tree proper is the balanced subtree over the triangle run, or an inner node over that
 *     and the balanced subtree over the sphere run when both exist; a run of more than leaf_max records (the scene's,
 *     default 4) splits at begin + count / 2.  The shape depends on n_global, the two run lengths and leaf_max only; the
 *     rebuilt stream has its own node count (rtx_scene_rebuilt_counts).
 *   boxes: every node's box is the fold of the own boxes of its run, moved outwards by cull_delta, as for rtx_scene_pose.
 * Every posed call then runs over the rebuilt pose unchanged, and for rays without a zero direction component returns what
 * it returns over the refitted pose: only speed changes (DESIGN.md section 19 has which tree wins where).  Ties and hard
 * groups: rtx_scene_pose's rule over the rebuilt stream; with a reference tree (host variant) its leaves name positions of
 * the sorted array.  rtx_scene_pose_rebuilt_device outside the range rule: keys saturate, the permutation is still a
 * permutation and the shape is fixed, so the calls terminate; the values are unspecified.  Spheres stay as uploaded
 * (rtx_scene_pose_prims moves them) and the primitive count does not change. */
int rtx_scene_pose_rebuilt(RtxScene *scene, int device, const float *v0v1v2, const uint32_t *tie_rank /* may be NULL */,
                           uint32_t reference_tree, RtxStats *stats);
int rtx_scene_pose_rebuilt_device(RtxScene *scene, int device, const void *d_v0v1v2, const void *d_tie_rank /* may be NULL */,
                                  void *stream);
/* Host only, no device: the node count of the rebuilt stream. */
int rtx_scene_rebuilt_counts(const RtxScene *scene, uint32_t *out_n_nodes);
/* Host only, no device: the words a rebuilt pose makes.  out_keys, out_perm: one per record of the tree proper
 * (n_prims - n_global), in sorted order: the key, and the position in the uploaded array (rtx_scene_nodes' out_tri_order)
 * of the record that sorted position n_global + p holds; out_tris: n_prims x 16 words in sorted order; out_shade:
 * n_prims x 8 in Vec order, as rtx_scene_posed_records'; out_nodes: rtx_scene_rebuilt_counts' x 8, NodeRec word order, the
 * planes moved by cull_delta.  Each output may be NULL.  The vertices are not checked against the range rule. */
int rtx_scene_rebuilt_records(const RtxScene *scene, const float *v0v1v2, const uint32_t *tie_rank, uint64_t *out_keys,
                              uint32_t *out_perm, uint32_t *out_tris, uint32_t *out_shade, uint32_t *out_nodes);
/* Host only, no device: the aim kernels' output over a rebuilt pose for `eye`: rtx_scene_rebuilt_records' node words (their
 * planes moved by cull_delta once, there) in rtx_scene_aimed_nodes' order; a scene that aims nothing: those words as they
 * are.  out_aimed: rtx_scene_rebuilt_counts' x 8 words.  RTX_ERR_BAD_ARG for a NULL. */
int rtx_scene_rebuilt_aimed(const RtxScene *scene, const float *v0v1v2, const float eye[3], uint32_t *out_aimed);
/* Diagnostic: blocks and copies the rebuilt pose `device` holds back, in rtx_scene_rebuilt_records' layout, and the aim
 * kernels' output over it for `eye` (out_aimed: the rebuilt node count x 8; a scene that aims nothing: the pose's stream).
 * Each output may be NULL; eye may be NULL when out_aimed is.  RTX_ERR_BAD_ARG when the device holds no rebuilt pose.
 * On a rebuilt pose rtx_debug_pose's out_nodes and rtx_debug_pose_pipeline's out_aimed — sized by the uploaded node
 * count — do not apply: RTX_ERR_BAD_ARG when they are not NULL. */
int rtx_debug_pose_rebuilt(RtxScene *scene, int device, const float eye[3], uint32_t *out_perm, uint32_t *out_tris,
                           uint32_t *out_shade, uint32_t *out_nodes, uint32_t *out_aimed);

/* ---- A pose that states every field of a primitive: spheres move, colours change ------------------------------------------
 * rtx_scene_pose_prims / _device are rtx_scene_pose / _device — under RTX_POSE_REBUILT rtx_scene_pose_rebuilt / _device —
 * in every respect: one pose per scene and device (a new pose of any kind replaces the previous one and takes the pose's
 * aimed stream away), the ordering, the tie rule and reference_tree (the reference's own tree clusters the POSED sphere
 * boxes), stats (kernel_ms now includes the overlay kernel), every posed call over it unchanged, rtx_debug_pose /
 * rtx_debug_pose_rebuilt / rtx_debug_pose_pipeline to read it back.  Beside the triangles' vertices the pose may state
 *   spheres:    every sphere's origin and radius.  Its primitive record and the `normal` words of its shading record are
 *               restated by Sphere::new and get_bounding_box (sphere.rs:21-41) — the one text rtx_scene_create runs on the
 *               host: v0 = origin, e1[0] = radius * radius, e1[1] = radius, the own box = origin -+ radius, each rounded
 *               once; every other word is the uploaded record's.  Node boxes fold the posed boxes; under
 *               RTX_POSE_REBUILT a sphere's key comes from its posed box.
 *   rgb, sphere_rgb: the colour of every triangle / every sphere (the rgb words of the shading record).
 * Only the primitive count and the order of arms in the Vec stay fixed.  A NULL array means "as UPLOADED", never "as the
 * previous pose": a plain rtx_scene_pose after such a pose puts spheres and colours back.  Arrays of an arm the scene does
 * not have are not read (v0v1v2 may be NULL for a scene without triangles).  The struct and, for the host variant, the
 * arrays are read before the call returns; the device variant's arrays (device pointers, 4-byte aligned) must stay valid
 * until the kernels have run.
 * On the device one kernel runs ahead of the pose's own: it writes an overlay of the uploaded records (library-owned,
 * grow-only buffers beside the pose's) which the pose or rebuild kernels read where they read the uploaded ones.  Without
 * spheres only the shading half is made; with vertices alone nothing is launched.  rtx_scene_pose* never touch it.
 * RTX_ERR_BAD_ARG: a NULL scene or struct, a NULL v0v1v2 with triangles present, an unknown flag or reference_tree.
 * Range rule (host variant: RTX_ERR_UNSUPPORTED, decided before a device is looked for; device variant: a stated
 * precondition): the triangles' as rtx_scene_pose's; for a sphere all four values finite and all six box words
 * origin -+ radius, as rounded above, of magnitude at most rtx_scene_pose_bound.  A negative radius is taken as
 * rtx_scene_create takes it.  Colours are not checked, as rtx_scene_create does not check them. */
#define RTX_POSE_REBUILT 1u             /* the tree as rtx_scene_pose_rebuilt makes it; 0: refitted as rtx_scene_pose */
typedef struct RtxPosePrims {           /* pointers: host for rtx_scene_pose_prims, device for _device */
    const float *v0v1v2;                /* n_tris x 9, required when the scene has triangles */
    const float *spheres;               /* NULL (as uploaded) or n_spheres x 4: origin x,y,z, radius */
    const float *rgb;                   /* NULL (as uploaded) or n_tris x 3 */
    const float *sphere_rgb;            /* NULL (as uploaded) or n_spheres x 3 */
    const uint32_t *tie_rank;           /* NULL or one per Vec position, as rtx_scene_pose's */
} RtxPosePrims;
int rtx_scene_pose_prims(RtxScene *scene, int device, const RtxPosePrims *prims, uint32_t flags, uint32_t reference_tree,
                         RtxStats *stats);
int rtx_scene_pose_prims_device(RtxScene *scene, int device, const RtxPosePrims *prims, uint32_t flags, void *stream);
/* Host only, no device: the words such a pose makes.  flags 0: rtx_scene_posed_records' layout, out_keys and out_perm must
 * be NULL (RTX_ERR_BAD_ARG); RTX_POSE_REBUILT: rtx_scene_rebuilt_records' layout.  Each output may be NULL.  Nothing is
 * checked against the range rule. */
int rtx_scene_pose_prims_records(const RtxScene *scene, const RtxPosePrims *prims, uint32_t flags, uint64_t *out_keys,
                                 uint32_t *out_perm, uint32_t *out_tris, uint32_t *out_shade, uint32_t *out_nodes);
/* Host only, no device: the aim kernels' output over such a pose for `eye`: rtx_scene_posed_pipeline_records' out_aimed
 * (flags 0) or rtx_scene_rebuilt_aimed's (RTX_POSE_REBUILT).  RTX_ERR_BAD_ARG for a NULL. */
int rtx_scene_pose_prims_aimed(const RtxScene *scene, const RtxPosePrims *prims, uint32_t flags, const float eye[3],
                               uint32_t *out_aimed);

/* ---- A pose by affine moves made on the device: the vertices never leave it ---------------------------------------------------
 * rtx_scene_pose_moved / _device are rtx_scene_pose_prims / _device in every respect not named here: one pose per scene and
 * device, the pose's aimed stream taken away, the ordering, the tie rule and reference_tree, RTX_POSE_REBUILT, stats
 * (kernel_ms now includes the move kernel), every posed call over it unchanged.  What differs is where the vertices and the
 * spheres come from: the device makes them from the scene's geometry AS CREATED (the "rest" geometry: RtxSceneDesc.v0v1v2
 * and .spheres as given, kept by rtx_scene_create and uploaded once per scene and device with the first such pose) and a
 * small set of affine maps, "moves"; every primitive names the move it follows, or none.  The per-call input of a rigid
 * animation is then 48 bytes per move, not 36 bytes per triangle.
 * The statement (scene_prep.h: move_statement, one text for the host and the device compiler, no contraction):
 *   a point p under move m (12 floats):  out[r] = ((m[4r] * p0 + m[4r+1] * p1) + m[4r+2] * p2) + m[4r+3]  for r = 0, 1, 2 —
 *     three products and three sums in this order, each rounded to f32 once;
 *   a triangle: its three vertices each; a sphere: its origin, and radius * radius_scale[g], one product (radius_scale NULL:
 *     the radius copied);
 *   group RTX_MOVE_NONE: the primitive keeps its created words bit for bit.  That is NOT the identity matrix, which turns a
 *     -0.0 coordinate into +0.0 (-0.0 * 1 + 0 * y + 0 * z + 0 = +0.0); RTX_MOVE_NONE keeps the sign;
 *   a group value >= n_moves other than RTX_MOVE_NONE: RTX_ERR_BAD_ARG from the host variant, which reads the array; the
 *     statement and the kernel take it as RTX_MOVE_NONE — `moves` and `radius_scale` are never indexed with a value that
 *     has not been compared against n_moves, whatever a device array holds.
 * Triangle::new, get_bounding_box and Sphere::new then run on these values as for any pose: a moved pose is
 * rtx_scene_pose_prims with the arrays rtx_scene_moved_prims states, word for word.
 * On the device one kernel runs ahead of the overlay and pose kernels and writes two library-owned grow-only buffers
 * (n_tris x 9 and n_spheres x 4 floats), which stand where a caller's v0v1v2 and spheres stand.  The host variant copies
 * moves, group, radius_scale and the colour arrays to the device per call; the device variant's arrays (device pointers,
 * 4-byte aligned) must stay valid until the kernels have run.
 * RTX_ERR_BAD_ARG (host variant: all decided before a device is looked for): a NULL scene or struct, a NULL moves, n_moves 0
 * or above 65,536, an unknown flag or reference_tree, a bad group value (above).  Range rule (host variant:
 * RTX_ERR_UNSUPPORTED, decided before a device is looked for — the host runs the statement and applies
 * rtx_scene_pose_prims' rule to its output, so a non-finite entry of a move that is followed fails here, and so does turning
 * a ground whose corner then leaves rtx_scene_pose_bound; device variant: a stated precondition).  The reference's own
 * tree (host variant) is built from the statement's output. */
#define RTX_MOVE_NONE 0xFFFFFFFFu      /* this primitive stays as uploaded: its words are copied, no arithmetic */
typedef struct RtxPoseMoves {          /* 56 bytes, alignment 8; pointers: host for the host call, device for _device */
    uint32_t n_moves;                  /* 1 ... 65,536 */
    const float *moves;                /* n_moves x 12: a 3 x 4 map, row major: rows of A, then the row's translation */
    const uint32_t *group;             /* NULL (every primitive follows move 0) or one per Vec position */
    const float *radius_scale;         /* NULL (radii as uploaded) or n_moves: a sphere's radius times this */
    const float *rgb, *sphere_rgb;     /* as RtxPosePrims': NULL = as uploaded */
    const uint32_t *tie_rank;          /* as RtxPosePrims' */
} RtxPoseMoves;
int rtx_scene_pose_moved(RtxScene *scene, int device, const RtxPoseMoves *moves, uint32_t flags /* RTX_POSE_REBUILT or 0 */,
                         uint32_t reference_tree, RtxStats *stats);
int rtx_scene_pose_moved_device(RtxScene *scene, int device, const RtxPoseMoves *moves, uint32_t flags, void *stream);
/* Host only, no device: the vertices and spheres such a pose makes (either output may be NULL): n_tris x 9 and
 * n_spheres x 4 floats.  RTX_ERR_BAD_ARG: a NULL scene, struct or moves, n_moves out of range.  Group values are taken as
 * the statement takes them; nothing is checked against the range rule. */
int rtx_scene_moved_prims(const RtxScene *scene, const RtxPoseMoves *moves, float *out_v0v1v2, float *out_spheres);
/* Diagnostic: blocks and copies back the arrays the move or skin kernel last wrote on `device` (either may be NULL);
 * RTX_ERR_BAD_ARG when neither ever ran there, or when a host pose of another kind has since reused the buffers. */
int rtx_debug_moved_prims(RtxScene *scene, int device, float *out_v0v1v2, float *out_spheres);

/* ---- A skinned pose: weighted moves per triangle corner, made on the device -------------------------------------------------
 * A moved pose lets a PRIMITIVE follow one move; a mesh that bends needs every CORNER to blend several.  A skin is bound to
 * the scene once — per triangle corner four move indices ("bones") and four weights, per sphere one move index — and a
 * skinned pose then takes only the moves: 48 bytes per move and frame, as a moved pose does, and nothing of the scene's size.
 * The statement for one corner (scene_prep.h: skin_statement, one text for the host and the device compiler, no
 * contraction), with p the corner as created:
 *   all four bones >= n_moves (RTX_MOVE_NONE is such a value): the corner keeps its created words bit for bit — no
 *     arithmetic, so the sign of a -0.0 survives; this is how the ground stays put;
 *   otherwise q_k = p under move bones[k] by rtx_scene_pose_moved's statement (a bone that is not below n_moves: q_k = p
 *     itself), and out[r] = ((w0 * q0[r] + w1 * q1[r]) + w2 * q2[r]) + w3 * q3[r] for r = 0, 1, 2 — four products and three
 *     sums in this order, each rounded to f32 once.  A slot of weight 0 still takes part: 1 * -0.0 + 0 * x is +0.0.
 *   Weights are taken as given: not normalised, not required to sum to 1; a weighted RTX_MOVE_NONE slot blends towards the
 *     rest position.  `moves` is never indexed with a value that has not been compared against n_moves.
 *   A sphere follows sphere_bone[s] exactly as a moved pose's sphere follows group[its position], radius_scale included.
 * rtx_scene_skin copies the arrays into the scene (host memory kept: 96 bytes per triangle and 4 per sphere — taking the
 * arrays per call instead would cost more per frame than the vertices they replace), replaces any previous skin and records
 * the largest bone other than RTX_MOVE_NONE; a NULL skin unbinds.  Like create and destroy it is not re-entrant per handle:
 * no other call on the scene may run beside it.  It touches no device and no pose that stands on one: each device uploads
 * the skin (library-owned, grow-only, 16-byte aligned buffers) with its first skinned pose after a bind.
 * RTX_ERR_BAD_ARG: a NULL scene, NULL bones or weights with triangles present.  RTX_ERR_UNSUPPORTED: a weight that is not
 * finite.  On an error the previous skin stays bound.
 * rtx_scene_skin_bound: 1 when a skin is bound, 0 when not (RTX_ERR_BAD_ARG for a NULL scene); *out_max_bone (may be NULL):
 * the largest bone other than RTX_MOVE_NONE over corners and spheres, 0 when there is none or no skin.
 * rtx_scene_pose_skinned / _device / rtx_scene_skinned_prims are rtx_scene_pose_moved / _device / rtx_scene_moved_prims in
 * every respect not named here (stats: kernel_ms includes the skin kernel; rtx_debug_moved_prims reads its arrays).  What
 * differs: moves->group must be NULL (the skin names the moves) and a skin must be bound, else RTX_ERR_BAD_ARG; the host
 * variant also returns RTX_ERR_BAD_ARG when n_moves <= the bind's largest bone (an O(1) check) and RTX_ERR_UNSUPPORTED by
 * the range rule over the statement's output, all before a device is looked for, and copies moves, radius_scale and the
 * colour arrays per call, nothing else.  For the device variant both are stated preconditions: outside them the call
 * still terminates and indexes nothing unchecked; the values are unspecified. */
typedef struct RtxSkin {               /* 24 bytes, alignment 8; host pointers */
    const uint32_t *bones;             /* n_triangles x 3 x 4: per corner (v0, v1, v2 in RtxSceneDesc.v0v1v2 order, spheres skipped) */
    const float *weights;              /* n_triangles x 3 x 4 */
    const uint32_t *sphere_bone;       /* NULL (every sphere RTX_MOVE_NONE) or n_spheres */
} RtxSkin;
int rtx_scene_skin(RtxScene *scene, const RtxSkin *skin);
int rtx_scene_skin_bound(const RtxScene *scene, uint32_t *out_max_bone);
int rtx_scene_pose_skinned(RtxScene *scene, int device, const RtxPoseMoves *moves, uint32_t flags /* RTX_POSE_REBUILT or 0 */,
                           uint32_t reference_tree, RtxStats *stats);
int rtx_scene_pose_skinned_device(RtxScene *scene, int device, const RtxPoseMoves *moves, uint32_t flags, void *stream);
int rtx_scene_skinned_prims(const RtxScene *scene, const RtxPoseMoves *moves, float *out_v0v1v2, float *out_spheres);

/* A resampled scene: the sample table of an existing scene replaced (the reference draws a new one for every render(),
 * main.rs:253-265).  Every later call on the scene — render, frame, tiles, view, view rows, shade, their lit and posed forms —
 * returns what it returns on a scene created from the same RtxSceneDesc with the new table, byte for byte and word for word.
 * rtx_scene_resample: `samples` is n_samples interleaved pairs, as RtxSceneDesc.samples; copied before the call returns.
 * rtx_scene_reseed: the table is rtxh_gen_samples(seed, n_pairs), word for word: draw i of 2 * n_pairs has the splitmix64
 *   state seed + (i + 1) * 0x9E3779B97F4A7C15 mod 2^64, mixed as rtxh_gen_samples mixes it, and the value
 *   (float)(uint32_t)(z >> 40) * 2^-24.  The table is never made on the host: the call does work proportional to nb_ray *
 *   nb_light_sample and none proportional to n_pairs, and each device makes its copy with a kernel (rtx_samples.hip) from the
 *   seed, so nothing of the table's size crosses the bus.
 * Both are host only and touch no device; like rtx_scene_skin they are not re-entrant per handle: no other call on the
 * scene may run beside them.  They re-derive what rtx_scene_create derives from the table, with create's own code: the light
 * points, the light tour and order, the light boxes and the shaft margin (rtx_scene_light_points, rtx_scene_light_order and
 * the _for calls answer for the new table at once).  KEPT AS CREATED: the prediction of the long primary walks
 * (rtx_scene_probe_long, which widened its frusta by the created table's range) — an ordering hint on which no byte
 * depends.  Not read from the table and so left alone: the gamma thresholds, the trees, the rest geometry, the skin, any pose
 * that stands on a device and the aimed streams.
 * RTX_ERR_BAD_ARG: a NULL scene, NULL samples, a count of 0.  RTX_ERR_UNSUPPORTED: the re-derived shaft margin is not
 * finite — rtx_scene_create's own rule: the calls accept exactly the tables create accepts.  RTX_ERR_OOM.  On any error the
 * scene stays exactly as it was.
 * Each device catches up in the first call of any kind on it after a replacement (rtx_scene_upload included), before that
 * call enqueues anything: it waits for the device (hipDeviceSynchronize: a launch on any stream may still read the old
 * table), replaces its table — a caller's by a copy, a seeded one by the kernel — and re-uploads the small light arrays.
 * Synchronous, as an upload is.  rtx_render_frame catches up every device it names before its first launch.
 * rtx_scene_samples: host only; copies `count` pairs of the scene's current table from pair `first` (a seeded table's pairs
 *   are computed, whatever its size).  RTX_ERR_BAD_ARG: a NULL scene, a NULL out with count != 0, first + count > the
 *   table's pairs.
 * rtx_debug_samples: the same range read back from `device`'s table, after the device caught up; blocks.
 * RtxSceneInfo.sample_bytes is 8 * the pair count for either kind of table. */
int rtx_scene_resample(RtxScene *scene, const float *samples, uint32_t n_samples);
int rtx_scene_reseed(RtxScene *scene, uint64_t seed, uint32_t n_pairs);
int rtx_scene_samples(const RtxScene *scene, uint64_t first, uint32_t count, float *out);
int rtx_debug_samples(RtxScene *scene, int device, uint64_t first, uint32_t count, float *out);

/* ---- The mean of N frames, accumulated on the device ---------------------------------------------------------------------------
 * One frame is one ray per pixel (nb_ray of them) and the table's light points: noisy and aliased, which is why the reference
 * draws a new table for every render() (main.rs:253-265).  These calls average N frames without a byte of a frame crossing
 * the bus and without changing the scene.
 *
 * THE STATEMENT.  An accumulator record is an RtxAccumPixel.  Adding frame k's RtxPixelShade record `s` to it:
 *   first:      sum[c] = s.linear[c], copied bit for bit; hit_frames = (s.hits != 0).  The old content is not read.
 *   otherwise:  sum[c] = sum[c] + s.linear[c], one f32 addition per channel; hit_frames += (s.hits != 0), a u32 addition.
 * Resolving it over n_frames gives an RtxPixelShade: linear[c] = sum[c] / (float)n_frames, ONE correctly rounded f32
 * division (not a product with a reciprocal); rgb8[c] the byte the frame's own pixel store gives that value, through the
 * scene's 256 gamma thresholds (rtx_scene_gamma_thresholds; -inf is byte 255, a NaN and every other negative value byte 0);
 * hits = min(hit_frames, 255): in how many frames the pixel had a hit.  Host and device compile one text (scene_prep.h:
 * accum_add_statement, accum_resolve_statement) without contraction and agree word for word.
 *
 * rtxh_accum_add / rtxh_accum_resolve: the two statements over arrays, host only, no device.  RTX_ERR_BAD_ARG: a NULL array
 * (a resolve: thr256 or accum, and both outputs NULL), n_frames == 0 or > 65,536.  n == 0: RTX_OK, nothing read or written.
 *
 * rtx_accum_add_device / rtx_accum_resolve_device: the same over device arrays, one kernel each (rtx_accum.hip),
 * asynchronous on `stream`.  d_shade of an add: records from ANY call that writes RtxPixelShade (rtx_render_view_device,
 * rtx_shade_rays_device, their lit and posed forms) — how a caller accumulates frames that differ in pose, eye or light:
 * motion blur, depth of field.  RTX_ERR_BAD_ARG: a NULL scene or array (a resolve: d_accum, and both outputs NULL), a pointer
 * other than d_rgb that is not 16-byte aligned (d_rgb may have any alignment), n_frames == 0 or > 65,536.  n == 0: RTX_OK,
 * nothing launched, no device needed.  They use no library buffer: no ordering rule ties them to other calls.  A resolve
 * reads the scene's thresholds and uploads the scene (synchronously) first if needed.
 *
 * rtx_render_view_mean: the mean of n_frames frames of a view, frame k rendered under the table
 * rtxh_gen_samples(seeds[k], n_pairs).  It is rtx_render_view_lit — with RTX_MEAN_POSED rtx_render_view_posed with that
 * light — in every respect not named here: the view and light argument checks, the empty rectangle (RTX_OK, nothing
 * written, stats zeroed, no device needed), RTX_ERR_UNSUPPORTED for a light vertex that is not finite (decided on the host),
 * RTX_ERR_BAD_ARG when posed and the device holds no pose.  light == NULL: the scene's own triangle and count;
 * nb_light_sample == 0: the scene's count.  Further RTX_ERR_BAD_ARG: NULL seeds, n_frames == 0 or > 65,536, n_pairs == 0, an
 * unknown flag, both outputs NULL (host variant), NULL or misaligned d_accum (device variant; its two outputs may both be
 * NULL: the sums stay in d_accum for a later rtx_accum_resolve_device).  seeds is read before the call returns.
 * Record p is the resolve of the adds, in frame order, of rtx_render_view_lit's record p on a scene created from the same
 * RtxSceneDesc with table rtxh_gen_samples(seeds[k], n_pairs): the ordered sum of the reference's render_pixel over N
 * scenes, divided once, then Color::to_rgba.  n_frames == 1: that frame's record, hits clipped to 0 or 1.
 * Per frame, all on the call's stream with no host wait between frames: the seeded table made by the sample-table kernel
 * into a library-owned scratch table (never the scene's), the light points of the call's light over that table, the view
 * kernel with its argument block's table and light points swapped, writing library-owned scratch records, and the add;
 * after the last frame the resolve.  THE SCENE IS NOT WRITTEN: its table, light arrays, pose, skin and aimed streams stay, and
 * every later call returns what it returned before.  The scratch table and records and the light points are library-owned
 * per device and grow only (growing waits for the device): device-resident launches on one device must be ordered on one
 * stream, and the host entry points wait (by an event) for the most recent of them, as for the lit calls.
 * stats (host variant; may be NULL): the counters are the sums over the frames, primary_rays = n_frames * nx * ny * nb_ray,
 * kernel_ms the whole chain. */
typedef struct RtxAccumPixel {   /* 16 bytes, 16-byte aligned on the device: one 16-byte load, one 16-byte store */
    float    sum[3];             /* the ordered f32 sum of the frames' linear colours */
    uint32_t hit_frames;         /* frames in which the pixel had a closest hit */
} RtxAccumPixel;
#define RTX_MAX_MEAN_FRAMES 65536u
#define RTX_MEAN_POSED 1u
int rtxh_accum_add(uint32_t n, const RtxPixelShade *shade, RtxAccumPixel *accum, uint32_t first);
int rtxh_accum_resolve(const float thr256[256], uint32_t n, const RtxAccumPixel *accum, uint32_t n_frames,
                       uint8_t *out_rgb /* NULL or n*3 */, RtxPixelShade *out_shade /* NULL or n */);
int rtx_accum_add_device(RtxScene *scene, int device, uint32_t n, const void *d_shade, void *d_accum, uint32_t first,
                         void *stream);
int rtx_accum_resolve_device(RtxScene *scene, int device, uint32_t n, const void *d_accum, uint32_t n_frames, void *d_rgb,
                             void *d_shade, void *stream);
int rtx_render_view_mean(RtxScene *scene, int device, const RtxView *view, const RtxLight *light /* NULL = the scene's */,
                         uint32_t flags, const uint64_t *seeds, uint32_t n_frames, uint32_t n_pairs, uint8_t *out_rgb,
                         RtxPixelShade *out_shade, RtxStats *stats);
int rtx_render_view_mean_device(RtxScene *scene, int device, const RtxView *view, const RtxLight *light, uint32_t flags,
                                const uint64_t *seeds, uint32_t n_frames, uint32_t n_pairs, void *d_accum, void *d_rgb,
                                void *d_shade, void *stream);

/* ---- the render pipeline's linear output: RtxPixelShade records ------------------------------------------------------------
 * rtx_render_view_rows, _lit and _posed write RGB8.  These two write, for the same rows, what rtx_render_view_lit (with
 * RTX_ROWS_POSED: rtx_render_view_posed) writes to out_shade for the same view and light: record (y - y0) * width + x is the
 * pixel's 16 bytes — `linear`, the three ordered f32 sums, bit for bit (a NaN stands for any NaN); `rgb8`, the bytes
 * rtx_render_view_rows* gives; `hits`, the number of the pixel's nb_ray rays with a closest hit, saturating at 255.  One
 * pair of functions with the light (NULL: the scene's) and the geometry (flags) as arguments.
 * In every other respect a call is its byte twin — rtx_render_view_rows / _device for a NULL light and no flag,
 * rtx_render_view_rows_lit / _device for a light, rtx_render_view_rows_posed / _device with RTX_ROWS_POSED: full width only,
 * the eye's range rule and the light's rules (RTX_ERR_UNSUPPORTED) decided before a device is looked for, ny == 0 (RTX_OK,
 * stats zeroed, no device needed), stats and kernel_ms, rtx_launch_timings and rtx_debug_tile_descs, no capture and replay,
 * launches on one device ordered on one stream, the host variant waiting for the lit and pose uses and the device-resident one
 * marking them, RTX_ERR_BAD_ARG when RTX_ROWS_POSED is given and `device` holds no pose.  It launches the RECORD FORMS of
 * the three kernels that store a pixel (namespace rtxo: the same bodies, one 16-byte store per pixel in place of three byte
 * stores) and leaves every later call on the scene unchanged.
 * Its own rules: RTX_ERR_BAD_ARG for a flag other than RTX_ROWS_POSED, for a d_shade that is NULL or not 16-byte aligned,
 * and for d_bytes < ny * width * 16. */
#define RTX_ROWS_POSED 1u
int rtx_render_view_rows_shade(RtxScene *scene, int device, const RtxView *view, const RtxLight *light /* NULL = the scene's */,
                               uint32_t flags /* RTX_ROWS_POSED or 0 */, RtxPixelShade *out_shade, RtxStats *stats);
int rtx_render_view_rows_shade_device(RtxScene *scene, int device, const RtxView *view, const RtxLight *light, uint32_t flags,
                                      void *d_shade, size_t d_bytes, void *stream, uint64_t *d_counters);

/* ---- the mean of N frames through the render pipeline ---------------------------------------------------------------------
 * rtx_render_view_mean / _device (above) with the pipeline's record launch in the view kernel's place.  For a full-width
 * rectangle (x0 == 0, nx == width) the outputs and the accumulator are rtx_render_view_mean's / _device's, word for word: the
 * adds are ordered, the division is made once, the scene is not written.  Argument checks: the mean call's, then full width
 * (RTX_ERR_BAD_ARG), then — decided on the host, before a device is looked for — the eye's range rule, a light with a
 * vertex that is not finite, and a frame whose shaft margin is not finite (RTX_ERR_UNSUPPORTED).  Stats are the sums over the
 * frames.  Per frame k, on the call's stream, with no host wait between frames: the sample-table kernel over (seeds[k],
 * n_pairs) into the mean's scratch table; the light's points, tour and boxes over that table by rtx_render_view_rows_lit's
 * kernels (light == NULL: the scene's own triangle and count, since every frame's points differ); a record launch
 * (rtx_render_view_rows_shade's kernels) into the mean's scratch records, its argument block's table, table length and the
 * light's five fields swapped; the add.  The aim kernels run once: there is one eye.  After the last frame the resolve.
 * The shaft margin of a frame's light points is made on the host from the seed, in closed form over the nb_ray * count
 * entries the points read (n_frames * nb_ray * count point statements per call); rtx_scene_light_walk_seeded reads it back,
 * host only: its outputs are rtx_scene_light_walk_for's on a scene reseeded with (seed, n_pairs), light == NULL: the
 * scene's own.  Ordering: the scratch buffers, the light buffers (the lit-rows buffers among them) and, when posed, the pose
 * are guarded as rtx_render_view_mean's are. */
int rtx_render_view_rows_mean(RtxScene *scene, int device, const RtxView *view, const RtxLight *light /* NULL = the scene's */,
                              uint32_t flags /* RTX_MEAN_POSED or 0 */, const uint64_t *seeds, uint32_t n_frames,
                              uint32_t n_pairs, uint8_t *out_rgb, RtxPixelShade *out_shade, RtxStats *stats);
int rtx_render_view_rows_mean_device(RtxScene *scene, int device, const RtxView *view, const RtxLight *light, uint32_t flags,
                                     const uint64_t *seeds, uint32_t n_frames, uint32_t n_pairs, void *d_accum, void *d_rgb,
                                     void *d_shade, void *stream);
int rtx_scene_light_walk_seeded(const RtxScene *scene, const RtxLight *light /* NULL = the scene's */, uint64_t seed,
                                uint32_t n_pairs, uint32_t *out_order, float *out_boxes, float *out_shaft_delta);

/* ---- The adaptive mean of N frames: tiles stop once their noise estimate is met ------------------------------------------------
 * rtx_render_view_mean gives every pixel the same N frames.  These calls keep a second moment per pixel and a noise estimate
 * per 8 x 8 tile of the RECTANGLE (tiles row by row over ceil(nx/8) x ceil(ny/8), as rtx_render_view's wavefronts: tile
 * (tx, ty) holds pixels [8tx, 8tx+8) x [8ty, 8ty+8) of the rectangle, cut at its right and bottom edges), and a frame's
 * launches skip the tiles whose estimate is already good enough.  Deterministic: every word below is stated.
 *
 * THE STATEMENT.  A moment record is an RtxMomentPixel.  Adding frame k's RtxPixelShade record `s` (l = s.linear) to it:
 *   first:      sum[c] = l[c], copied bit for bit; sumsq[c] = l[c] * l[c]; hit_frames = (s.hits != 0); frames = 1.  The old
 *               content is not read.
 *   otherwise:  sum[c] = sum[c] + l[c]; sumsq[c] = sumsq[c] + (l[c] * l[c]), the product rounded to f32 first, never an
 *               FMA; hit_frames += (s.hits != 0); frames += 1.
 * sum and hit_frames are RtxAccumPixel's, word for word.  A pixel's error, with fn = (float)frames, per channel:
 *   mean = sum[c] / fn;  q = sumsq[c] / fn;  v = q - (mean * mean), the product rounded first;  v = v > 0 ? v : 0 (a NaN or
 *   a negative rounding residue becomes 0);  e_c = v / fn
 * and the error is max(max(e_0, e_1), e_2) by `a < b ? b : a`: the (biased) variance of the mean of the noisiest channel,
 * never NaN, never negative.  A TILE'S ERROR is the maximum of its pixels' errors over the pixels inside the rectangle,
 * starting from +0.0; the order does not matter.  A tile's state is an RtxTileState {frames, err}, written by the add that
 * gave the tile a frame.  A tile is STOPPED under a rule when
 *   state.frames >= rule.min_frames && state.err <= rule.max_variance
 * — there is no separate "stopped" word: the masked view launch and the add both evaluate this from the 8-byte state.  A
 * stopped tile is neither rendered nor added to, its moments and its state keep their words, so within a call stopping is
 * final; a later RTX_ADAPT_CONTINUE call with a stricter rule resumes tiles by itself.  Under `first` the state is not read:
 * every tile is live.  Resolving a record gives an RtxPixelShade: linear[c] = sum[c] / (float)frames, ONE correctly rounded
 * division by the pixel's OWN count; rgb8 and hits as rtx_accum_resolve's.  Host and device compile one text (scene_prep.h:
 * moment_add_statement, moment_error_statement, tile_stopped, moment_resolve_statement) without contraction and agree word
 * for word.  Outside the contract for the DECISION: records that are not finite or whose squares overflow (the words are
 * still the statement's, host and device alike), frames == 0 in a resolve, more than 2^24 frames per pixel.
 * A TRAP: after one frame v is exactly 0 (mean = l, q = l * l), so min_frames == 1 stops every tile after frame 0 for ANY
 * max_variance.  min_frames >= 2 is the meaningful range.
 *
 * rtxh_moment_add / rtxh_moment_resolve: the statements over arrays, host only, no device.  An add takes the nx x ny
 * records of a rectangle (record y * nx + x), its moments and — tiles != NULL — its ceil(nx/8) * ceil(ny/8) tile states
 * and the rule; tiles == NULL (rule may be NULL too): every tile is live and no state is written, the plain moment
 * accumulator.  first != 0: moments and tiles are written, never read.  RTX_ERR_BAD_ARG: a NULL shade or moments, tiles
 * without a rule, a rule with min_frames == 0 or a max_variance that is negative or NaN, nx * ny > 2^28; a resolve: NULL
 * thr256 or moments, both outputs NULL.  nx * ny == 0 / n == 0: RTX_OK, nothing read or written.
 *
 * rtx_moment_add_device / rtx_moment_resolve_device: the same over device arrays, one kernel each (rtx_adapt.hip),
 * asynchronous on `stream`, no library buffer, no ordering rule.  d_shade: records from ANY call that writes RtxPixelShade,
 * the pipeline's rtx_render_view_rows_shade_device included.  RTX_ERR_BAD_ARG: the host statements' and a NULL scene, d_shade,
 * d_moments (or d_rgb and d_shade both NULL) or a pointer that is not aligned: 16 bytes for records and moments, 8 for d_tiles,
 * any for d_rgb.  An empty rectangle: RTX_OK, nothing launched, no device needed.  A resolve reads the scene's thresholds and
 * uploads the scene first if needed.
 *
 * rtx_render_view_adaptive / _device: rtx_render_view_mean / _device in every respect not named here — the argument checks,
 * the empty rectangle, the light's rules decided on the host, RTX_MEAN_POSED, THE SCENE IS NOT WRITTEN, the mean's scratch
 * table and records and the light buffers reused and guarded as the mean's are, seeds read before the call returns.  Further
 * RTX_ERR_BAD_ARG: a NULL rule, min_frames == 0, max_variance negative or NaN (+infinity is allowed), NULL or misaligned
 * d_moments or d_tiles (16 and 8 bytes; device variant).  Per frame k, on the call's stream, with no host wait between
 * frames: the sample-table kernel, the light points, the MASKED view launch (rtx_render_view's tile body behind the stopped
 * test, records only) into the scratch records, the moment add; after the last frame the resolve, where an output is asked
 * for.  All n_frames frames are always enqueued: once every tile has stopped the remaining launches' wavefronts return at
 * once.  With min_frames == n_frames no tile stops early and the outputs, sum and hit_frames are rtx_render_view_mean's.
 * RTX_ADAPT_CONTINUE (device variant only): d_moments and d_tiles hold an earlier call's state for the same rectangle; no
 * frame is a first one and seeds[k] are the NEXT frames' seeds — how an interactive caller refines in slices.
 * out_tiles (host variant, may be NULL): the tile states after the last frame; a tile's `frames` is its stop frame or
 * n_frames.  stats (host variant; it reads the tile states back): the counters are sums over the rendered tile-frames,
 * primary_rays = the sum over tiles of frames * pixels of the tile inside the rectangle * nb_ray. */
typedef struct RtxMomentPixel {   /* 32 bytes; 16-byte aligned on the device: two 16-byte loads, two stores */
    float    sum[3];              /* RtxAccumPixel.sum, word for word */
    uint32_t hit_frames;          /* RtxAccumPixel.hit_frames */
    float    sumsq[3];            /* ordered f32 sum of the frames' squared linear colours */
    uint32_t frames;              /* frames this pixel received */
} RtxMomentPixel;
typedef struct RtxTileState {     /* 8 bytes: one per 8x8 tile of the RECTANGLE, tiles row by row, as rtx_render_view's */
    uint32_t frames;              /* frames the tile received (= each of its pixels' frames) */
    float    err;                 /* the tile's noise estimate after its last add */
} RtxTileState;
typedef struct RtxAdaptRule { uint32_t min_frames; float max_variance; } RtxAdaptRule;
#define RTX_ADAPT_CONTINUE 2u
int rtxh_moment_add(uint32_t nx, uint32_t ny, const RtxPixelShade *shade, RtxMomentPixel *moments,
                    RtxTileState *tiles /* NULL ok */, uint32_t first, const RtxAdaptRule *rule /* NULL when tiles is */);
int rtxh_moment_resolve(const float thr256[256], uint32_t n, const RtxMomentPixel *moments,
                        uint8_t *out_rgb /* NULL or n*3 */, RtxPixelShade *out_shade /* NULL or n */);
int rtx_moment_add_device(RtxScene *scene, int device, uint32_t nx, uint32_t ny, const void *d_shade, void *d_moments,
                          void *d_tiles, uint32_t first, const RtxAdaptRule *rule, void *stream);
int rtx_moment_resolve_device(RtxScene *scene, int device, uint32_t n, const void *d_moments, void *d_rgb, void *d_shade,
                              void *stream);
int rtx_render_view_adaptive(RtxScene *scene, int device, const RtxView *view, const RtxLight *light /* NULL = the scene's */,
                             uint32_t flags /* RTX_MEAN_POSED or 0 */, const uint64_t *seeds, uint32_t n_frames,
                             uint32_t n_pairs, const RtxAdaptRule *rule, uint8_t *out_rgb, RtxPixelShade *out_shade,
                             RtxTileState *out_tiles /* may be NULL */, RtxStats *stats);
int rtx_render_view_adaptive_device(RtxScene *scene, int device, const RtxView *view, const RtxLight *light, uint32_t flags
                                    /* RTX_MEAN_POSED | RTX_ADAPT_CONTINUE */, const uint64_t *seeds, uint32_t n_frames,
                                    uint32_t n_pairs, const RtxAdaptRule *rule, void *d_moments, void *d_tiles, void *d_rgb,
                                    void *d_shade, void *stream);

/* ---- The adaptive mean through the render pipeline: a stopped tile is not scheduled ------------------------------------------
 * rtx_render_view_rows_adaptive / _device: rtx_render_view_adaptive / _device (above) in every respect, with the pipeline's
 * MASKED record launch in the masked view kernel's place.  For a full-width rectangle (x0 == 0, nx == width) every output is
 * the view-kernel call's, word for word: moments, tile states with their stop frames, records and bytes.  Argument checks,
 * in this order: the adaptive call's; full width (RTX_ERR_BAD_ARG); then — decided on the host before a device is looked for,
 * as rtx_render_view_rows_mean does — the eye's range rule, a light with a vertex that is not finite, and a frame whose
 * shaft margin is not finite (RTX_ERR_UNSUPPORTED).  Per frame k, on the call's stream, with no host wait between frames: the
 * sample-table kernel; the light's points, tour and boxes; the masked record launch into the mean's scratch records (a first
 * frame: the unmasked record launch, rtx_render_view_rows_shade's); the moment add.  After the last frame the resolve.  The
 * aim kernels run once.  The masked launch is the record launch whose scheduling pass (namespace rtxn) reads, per 8 x 8 tile
 * of the rectangle, the tile's RtxTileState — tiles row by row, as everywhere above — and evaluates the stopped test: a
 * stopped tile gets a descriptor that schedules nothing (rtx_debug_tile_descs: class 0xFFFFFFFF, no hits, no flags, nothing
 * counted), makes no ray, stores no pixel, queues nothing and touches no counter, and so never reaches the shading pass or
 * the reference pass.  All n_frames frames are always enqueued; a frame in which every tile has stopped still runs the
 * light's kernels and the pipeline's four dispatches over empty lists.  The scene is not written; the scratch buffers, the
 * light buffers and, when posed, the pose are guarded as rtx_render_view_rows_mean's are; rtx_launch_timings and
 * rtx_debug_tile_descs see the frames' launches; no capture and replay.  stats (host variant): as rtx_render_view_adaptive's.
 *
 * rtx_render_view_rows_shade_masked_device: the building block, device-resident only — rtx_render_view_rows_shade_device
 * behind the mask.  d_tiles: ceil(width/8) * ceil(ny/8) RtxTileState written by an earlier launch on the stream (or by the
 * caller), 8-byte aligned.  A tile stopped under `rule` keeps the words its records in d_shade held; a live tile's records
 * are the unmasked call's, and d_counters receives the live tiles' counts alone.  A caller whose frames differ in pose, eye
 * or light pairs it with rtx_moment_add_device under the same states and rule: adaptive motion blur.  Further
 * RTX_ERR_BAD_ARG beyond the unmasked call's: a NULL d_tiles or one that is not 8-byte aligned, a NULL rule,
 * min_frames == 0, a max_variance that is negative or NaN. */
int rtx_render_view_rows_adaptive(RtxScene *scene, int device, const RtxView *view, const RtxLight *light /* NULL = the scene's */,
                                  uint32_t flags /* RTX_MEAN_POSED or 0 */, const uint64_t *seeds, uint32_t n_frames,
                                  uint32_t n_pairs, const RtxAdaptRule *rule, uint8_t *out_rgb, RtxPixelShade *out_shade,
                                  RtxTileState *out_tiles /* may be NULL */, RtxStats *stats);
int rtx_render_view_rows_adaptive_device(RtxScene *scene, int device, const RtxView *view, const RtxLight *light, uint32_t flags
                                         /* RTX_MEAN_POSED | RTX_ADAPT_CONTINUE */, const uint64_t *seeds, uint32_t n_frames,
                                         uint32_t n_pairs, const RtxAdaptRule *rule, void *d_moments, void *d_tiles, void *d_rgb,
                                         void *d_shade, void *stream);
int rtx_render_view_rows_shade_masked_device(RtxScene *scene, int device, const RtxView *view, const RtxLight *light,
                                             uint32_t flags /* RTX_ROWS_POSED or 0 */, const void *d_tiles,
                                             const RtxAdaptRule *rule, void *d_shade, size_t d_bytes, void *stream,
                                             uint64_t *d_counters);

/* Diagnostics: per 8x8 pixel tile of rows [row0,row0+nrows), RTX_WAVE_PROFILE_WORDS uint64 {node records
 * fetched, triangle records fetched, start, end, primary phase, shadow phase (slowest wavefront),
 * accumulation phase, reserved}, times in ticks of the 100 MHz device wall clock.  Call with
 * out == NULL to get the tile grid (*tiles_x, *tiles_y); out_tiles = capacity of out in tiles. */
#define RTX_WAVE_PROFILE_WORDS 8
int rtx_debug_wave_profile(RtxScene *scene, int device, uint32_t row0, uint32_t nrows, uint64_t *out,
                           size_t out_tiles, uint32_t *tiles_x, uint32_t *tiles_y);

/* Diagnostics: device time of the most recent launches on `device`, oldest first.  A launch is two passes — the
 * scheduling pass (probe_kernel + order_tiles_kernel: primary hits and the cost order of the tiles) and the
 * shading pass (shade_tiles_kernel: shadow rays, ordered sums, RGB8) — bracketed by HIP events on the launch's
 * stream; schedule_ms[i] / shade_ms[i] are their durations (schedule_ms = 0 for the single-kernel variants).
 * Blocks until those launches have completed.  Returns how many launches were written (<= max_launches and
 * <= RTX_TIMING_RING) or a negative RtxError. */
#define RTX_TIMING_RING 64
int rtx_launch_timings(RtxScene *scene, int device, int max_launches, float *schedule_ms, float *shade_ms);

/* Diagnostics: the tile descriptors the most recent launch on `device` left in the library's workspace, one per 8x8
 * tile of that launch, four uint32 each.  Tiles are numbered by 8 x 8 BLOCKS of tiles (64 x 64 pixels), blocks row by row
 * over ceil(tiles_x / 8) x ceil(tiles_y / 8) blocks, the tiles of a block row by row: tile number t is tile
 * (x, y) = ((t / 64 % blocks_x) * 8 + t % 8, (t / 64 / blocks_x) * 8 + t % 64 / 8); numbers whose (x, y) lies outside
 * the launch's tiles are padding (no hits).  Each descriptor: {cost class (0xFFFFFFFF: finished by the scheduling pass), primary
 * hits, flags (bit 0 sample-major numbering, bit 1 re-rendered by the reference walk, bits 8-15 entries of the tile's
 * cut), reserved}.  Call with out == NULL to get the count.  Blocks until the device is idle.  Returns the number of
 * tiles written (<= max_tiles) or a negative RtxError. */
int rtx_debug_tile_descs(RtxScene *scene, int device, uint32_t *out, size_t max_tiles);
/* Diagnostics: what the scheduling pass of the most recent launch on `device` left beside the descriptors, in
 * rtx_debug_tile_descs' tile numbering: out_hits, 64 x 12 words per tile (a tile's compacted hit records, or their compact
 * form when the descriptor's flags say so; words no hit of that launch wrote hold what earlier launches left), and
 * out_pix_slots, 64 words per tile (the hit record of each pixel, 0xFFFFFFFF: none; written for tiles with a hit).  Either
 * may be NULL; both NULL: the tile count.  Blocks until the device is idle.  Returns the tiles written or a negative RtxError. */
int rtx_debug_probe_records(RtxScene *scene, int device, uint32_t *out_hits, uint32_t *out_pix_slots, size_t max_tiles);

/* The long primary walks.  rtx_scene_create predicts, per 8 x 8 pixel tile of the scene's own frame (tile t = tile_y *
 * ceil(width / 8) + tile_x), how much of the primary rays' stream the tile's rays can pass: the weight of the records whose
 * stored box meets the frustum of the eye and the tile's pixels (widened by the sample table's range and one pixel), an
 * inner record 1, a leaf 1 + 3 x its primitive records.  Tiles of at least the threshold weight form the long list,
 * costliest first, at most min(tiles / 32, 1024); a list of fewer than 8 tiles is dropped.  The scheduling pass starts those tiles first, a workgroup each, and
 * walks their primary rays as four 4 x 4 pixel beams.  An ordering hint: every byte is what it is without it.  It applies
 * to rtx_render_rows, rtx_render_frame and rtx_render_tiles_device where the launch's tiles are tiles of the frame (the
 * share starts on a multiple of 8 rows and, unless it is one band, tile_rows is a multiple of 8); not to scenes of more
 * than 2^16 stream records, not to launches of more than 65,536 tiles (whose scheduling pass is bound by throughput), not
 * to the view calls and not to posed geometry.
 * rtx_scene_probe_long: host only; copies up to max_entries tile numbers and weights (either may be NULL; both NULL: the
 *   count) and the threshold; returns the entries written.
 * rtx_scene_probe_tile: host only; the weight of one tile and, out_met != NULL, one byte per record of
 *   rtx_scene_primary_nodes' stream, 1 where the tile's frustum meets the record (the root and the global triangles' leaf,
 *   which every walk takes untested, always).  Returns 1, or 0 when the scene predicts nothing (*out_weight = 0).  A call
 *   for tests: each one sets the stream's boxes up anew (time linear in the stream, whatever the tile).
 * rtx_debug_probe_split: for tests and A/B runs.  mode 0: the prediction (default); 1: no tile is long; 2: every tile of
 *   the frame is long.  Holds for the scene's later launches.  Returns the number of long-list workgroups the scene's most
 *   recent pipeline launch was handed (0: it ran one wavefront per tile throughout), or a negative RtxError. */
int rtx_scene_probe_long(const RtxScene *scene, uint32_t *out_tiles, uint32_t *out_weights, size_t max_entries,
                         uint32_t *out_threshold);
int rtx_scene_probe_tile(const RtxScene *scene, uint32_t tile_x, uint32_t tile_y, uint8_t *out_met /* n_nodes */,
                         uint32_t *out_weight);
int rtx_debug_probe_split(RtxScene *scene, uint32_t mode);

const char *rtx_strerror(int err);
int rtx_last_hip_error(void);

/* ---- prepared-scene read-back (host logic tests, no device needed) --------- */
/* out: n_light_points x 3 floats — Light::get_sample(T[(r*nb_ray+i) % n]) (src/main.rs:194-196) */
int rtx_scene_light_points(const RtxScene *scene, float *out);
/* host only, no device: the points of ANY light on this scene — nb_ray * n points x 3 floats, n the light's count or, for
   0, the scene's; point [r][i] = get_sample(T[(r*nb_ray + i) % n_samples]), the index in 64 bits.  The host statement of
   what the light kernel makes (rtx_debug_light_points); for rtx_scene_light's value it is rtx_scene_light_points bit for
   bit.  out may be NULL.  Returns the number of points, or a negative RtxError: RTX_ERR_BAD_ARG for a NULL scene or light
   and for nb_ray * n > 2^20.  Vertices are not checked: a coordinate that is not finite gives points that are not. */
int rtx_scene_light_points_for(const RtxScene *scene, const RtxLight *light, float *out);
/* out: n_light_points words — the order in which the shading pass WALKS the light samples of primary ray r: the samples
   are cut into batches of min(nb_light_sample, 128) consecutive ones, and word r*nb_light_sample + k is the sample index
   (0 <= index < nb_light_sample) at walk position k.  Every batch is a permutation of its own indices that starts with
   its first sample: a short tour of the light (nearest neighbour, then 2-opt).  The order of a pixel's additions is the
   reference's, by ascending sample index, whatever this order is. */
int rtx_scene_light_order(const RtxScene *scene, uint32_t *out);
/* host only, no device: what the walk kernels make for `light` on this scene (rtx_render_view_rows_lit), n its count or, for
   0, the scene's.  out_order: nb_ray * n words in rtx_scene_light_order's form.  Every batch is a permutation of its own
   indices that starts with its first sample, whatever the points hold, made by this scan in f32: D(a, b) =
   sqrtf((e0*e0 + e1*e1) + e2*e2), e_k = a_k - b_k; nearest neighbour from the batch's first point with `d < best` only (a
   NaN or infinite distance never wins; a step that nothing wins goes to the lowest index left); then first-improvement 2-opt
   on the open path, i ascending, then j ascending, reversing positions [i, j] when after < before, where before = D(i-1, i)
   [+ D(j, j+1)] and after = D(i-1, j) [+ D(i, j+1)] are f32 sums (the second term when j is not the path's end), at most 32
   passes, position 0 never moving.  It is not rtx_scene_light_order's scan, which measures in double.  out_boxes: nb_ray x
   6 floats, lo xyz and hi xyz of the ray's points by fmin / fmax from -+infinity (a NaN is ignored).  out_shaft_delta: the
   margin of the shaft test under this light, bit for bit rtx_scene_create's for rtx_scene_light's value.  Each output may
   be NULL.  Returns the number of points, or a negative RtxError: RTX_ERR_BAD_ARG as rtx_scene_light_points_for. */
int rtx_scene_light_walk_for(const RtxScene *scene, const RtxLight *light, uint32_t *out_order, float *out_boxes,
                             float *out_shaft_delta);
/* out: 256 floats; byte value of a linear channel x = number of thresholds b>=1 with thr[b] <= x */
int rtx_scene_gamma_thresholds(const RtxScene *scene, float *out256);
/* out: (n_tris + n_spheres) x 3 in Vec order: unit normal of a triangle (Triangle::new, triangle.rs:29),
   origin of a sphere (its normal is normalize(p_hit - origin), sphere.rs:93-95) */
int rtx_scene_normals(const RtxScene *scene, float *out);
/* the traversal stream: node records (8 dwords each) and the triangle order of the leaves */
int rtx_scene_nodes(const RtxScene *scene, uint32_t *out_dwords /* n_nodes*8 */, uint32_t *out_tri_order /* n_tris */);
/* the stream the PRIMARY rays walk: the same tree and the same n_nodes records as rtx_scene_nodes, of every node's children
   the one nearer the eye first (the shadow rays' stream puts the one farther from the light first); *out_own = 1 when the
   scene has such a stream of its own, 0 when the primary rays walk rtx_scene_nodes' stream (which is then what is copied) */
int rtx_scene_primary_nodes(const RtxScene *scene, uint32_t *out_dwords /* n_nodes*8 */, uint32_t *out_own);
/* host only, no device: the stream the primary rays of a view with this eye walk (rtx_render_view_rows): n_nodes*8 dwords,
   NodeRec word order as rtx_scene_nodes.  It is rtx_scene_nodes' stream with every plane moved outwards by cull_delta, in
   f32, as the device holds it, and below the tree proper's root the child nearer the eye first: of a node's children a
   (the next record) and b (named by info), with c_k = (0.5*lo_k + 0.5*hi_k) - eye_k and d2 = c_0^2 + c_1^2 + c_2^2 in
   double, a stays first unless d2(b) < d2(a).  The host statement of what the aim kernels make (rtx_debug_aimed_nodes);
   a scene without a primary stream of its own: the moved stream in its own order. */
int rtx_scene_aimed_nodes(const RtxScene *scene, const float eye[3], uint32_t *out_dwords);
/* the reference-tree stream (n_ref_nodes*8 dwords; leaf info = 0x80000000 | position in out_tri_order) */
int rtx_scene_ref_nodes(const RtxScene *scene, uint32_t *out_dwords);

/* ---- host helpers: the caller side of the seam, restated (rtxh_*) ---------- */
/* Camera::new, src/tracer/utils/camera.rs:17-35 */
void rtxh_camera_new(const float eye[3], const float look_at[3], const float up[3],
                     float u[3], float v[3], float w[3]);
/* import_obj, src/main.rs:114-149: returns the triangle count (>= 0) and a malloc'ed n x 9 array
 * in *v0v1v2 (free with rtxh_free), or a negative RtxError. */
int  rtxh_import_obj(const char *path, float **v0v1v2);
/* The same loader with what import_obj leaves out, each part opt-in so that flags = 0 is import_obj
 * bit for bit (the reference's own assets use none of it):
 *   RTXH_OBJ_SLASHES    face tokens "v/vt/vn", "v//vn", "v/vt": the vertex index is the part before the first '/'
 *   RTXH_OBJ_RELATIVE   negative indices count back from the vertices read so far (-1 = the last one)
 *   RTXH_OBJ_POLYGONS   faces with more than three vertices become a fan (v0,v1,v2), (v0,v2,v3), ...
 *                       (import_obj silently keeps the first three)
 *   RTXH_OBJ_MATERIALS  "mtllib f" / "usemtl m": a triangle takes the Kd of the current material, read from the
 *                       .mtl file beside the OBJ (import_obj gives every mesh triangle Color::new(1,1,1),
 *                       src/main.rs:146); unknown material or unreadable library: (1,1,1)
 * With any flag set, tokens are separated by runs of blanks and tabs (import_obj splits on every single space).
 * *rgb (may be NULL) receives a malloc'ed n x 3 array of colours.  Returns the triangle count or a negative RtxError. */
#define RTXH_OBJ_SLASHES   1u
#define RTXH_OBJ_RELATIVE  2u
#define RTXH_OBJ_POLYGONS  4u
#define RTXH_OBJ_MATERIALS 8u
#define RTXH_OBJ_ALL       15u
int  rtxh_import_obj_ex(const char *path, uint32_t flags, float **v0v1v2, float **rgb);
void rtxh_free(void *p);
/* rank of each primitive in the left-to-right leaf order of BoundingVolumeHierarchy::new
 * (bounding_volume_hierarchy.rs:173-226; O(n^2)): out_rank[i] for triangle i. */
int  rtxh_ref_leaf_rank(uint32_t n_tris, const float *v0v1v2, uint32_t *out_rank);
/* seeded stand-in for the thread_rng table (src/main.rs:260-265): splitmix64, 24-bit floats */
void rtxh_gen_samples(uint64_t seed, uint32_t n_pairs, float *out);
/* Places the packed rows of one share (row tiles first_tile, first_tile + tile_stride, ... of tile_rows rows, clipped to
 * the frame, one after another in `packed`: what rtx_render_tiles_device writes) into their rows of a height x width
 * RGB8 frame — the gather of src/main.rs:291-295 with disjoint row ranges in place of the Mutex<DynamicImage>. */
int  rtxh_scatter_tiles(uint8_t *frame, uint32_t height, uint32_t width, const uint8_t *packed, uint32_t first_tile,
                        uint32_t tile_stride, uint32_t tile_rows);
/* RGB8 PNG (what img.save(.., image::PNG) produces on decode, src/main.rs:313-315) */
int  rtxh_write_png(const char *path, uint32_t width, uint32_t height, const uint8_t *rgb);
/* BASELINE.json configs[4], "synthetic 1M-triangle random mesh": n_tris triangles whose centroid is uniform in
 * the big_bunny AABB [-92.4,59.7]x[32.7,183.4]x[-60.5,57.6] and whose vertices are centroid + uniform offsets
 * in [-1,1]^3; draws from splitmix64(seed) as in rtxh_gen_samples, 12 per triangle
 * (centroid xyz, then v0 xyz, v1 xyz, v2 xyz); zero-area triangles are redrawn.  out: n_tris x 9. */
int  rtxh_synthetic_mesh(uint64_t seed, uint32_t n_tris, float *out_v0v1v2);

#ifdef __cplusplus
}
#endif
#endif /* RTX_H */
