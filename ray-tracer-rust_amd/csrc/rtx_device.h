// rtx_device.h — kernel argument blocks and the launcher, shared by rtx_kernel.hip and rtx_api.cpp.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "scene_prep.h"

// 1: the ablation library (librtx_ablation.so), which holds the earlier kernel forms beside the product's pipeline
#ifndef RTX_ABLATION
#define RTX_ABLATION 0
#endif

namespace rtx {

// Everything the kernel reads, resident in HBM for the life of the upload.
// Passed by value (kernarg segment -> SGPRs).
struct DeviceScene {
    // (the node streams are uploaded with their planes moved outwards by PreparedScene::cull_delta: the multiply-based box
    //  test then needs no widening of its own, rtx_traverse.hpp: box_mask)
    const NodeRec  *nodes;         // (n_nodes + 1) x 32 B, pre-order with skip links; last = zeroed sentinel
    const NodeRec  *primary_nodes; // the same tree, the same size, nearest-to-the-eye child first: the primary rays' stream (= nodes when there is none)
    const float    *light_tour;    // nb_ray x nb_light x 4: the light points in the order shade_tiles_kernel walks them
                                   // (PreparedScene::light_tour: x, y, z, the sample's index within its batch as bits).
                                   // In the slot the four-child tree's pointer had, whose count n_wide below stays unused:
                                   // the kernels' register allocation depends on the argument layout (without the two the
                                   // SGPR spill counts of probe_kernel and shade_tiles_kernel move by up to 12 either way)
    const NodeRec  *ref_nodes;     // (n_ref_nodes + 1) x 32 B: the reference's own tree, or NULL
    const TriRec   *tris;          // n_tris x 64 B, leaf order
    const ShadeRec *shade;         // n_tris x 32 B, caller order
    const TriRec   *planes;        // n_global x 64 B: plane data of the global triangles (PreparedScene::global_planes), or NULL
    const float2   *samples;       // n_samples x (s.0, s.1)
    const float    *light_points;  // nb_ray x nb_light x 3
    const float    *gamma_thr;     // 256
    const float    *light_boxes;   // nb_ray x 6: bounding box (lo xyz, hi xyz) of the light points of primary ray r
    uint32_t n_nodes, n_ref_nodes, n_samples, n_wide;
    uint32_t width, height;
    uint32_t nb_ray, nb_light;
    uint32_t n_global;             // > 0: primitive records [0, n_global) are tested by every walk up front, the tree proper starts at node 2
    uint32_t n_spheres;            // > 0: some leaves carry kSphereFlag: the fused kernel with the Sphere arm compiled in is launched
    float eye[3], cu[3], cv[3], cw[3];
    float distance;
    float shaft_delta;             // margin of the tile shaft test in position units (PreparedScene::shaft_delta)
    uint32_t cut_max_nodes;        // scenes of more stream records than this do not cut per tile: every chunk walks the whole
                                   // stream.  kCutMaxNodes in librtx.so; librtx_ablation.so reads RTX_CUT_MAX_NODES (0 = never
                                   // cut) so that a test can render ONE scene both ways and compare the bytes
    uint32_t n_prims;              // primitive records (triangles + spheres)
    uint32_t j1_mode;              // librtx_ablation.so only (RTX_J1, rtx_j1_ablation.hpp): 0 = the shipped pipeline; librtx.so: 0
};
constexpr uint32_t kCutMaxNodes = 1u << 16;
static_assert(kCutMaxNodes == kProbeSplitMaxNodes, "a scene predicts long tiles exactly when it cuts per tile");

// The scene's prediction of its long primary walks (PreparedScene::long_tiles, long_bits) on the device: n_long tile
// numbers of the scene's own frame, costliest first, then a bit per frame tile.  probe_kernel's argument alone, behind its
// others, and not a field of DeviceScene: the block every kernel is handed keeps its layout, and with it every other
// kernel its code.  n_long = 0 (words is not read): the pass runs one wavefront per tile throughout.  x_range, y_range:
// the rectangle of frame tiles around the listed ones, lowest | highest << 16 (probe_split_ranges): a tile outside it does
// not look its bit up.
struct ProbeSplit {
    const uint32_t *words;
    uint32_t n_long;
    uint32_t x_range, y_range;
};
// fills x_range and y_range for a list of n frame tile numbers; false (nothing split) when a tile coordinate needs more than 16 bits
inline bool probe_split_ranges(const uint32_t *tiles, uint32_t n, uint32_t tiles_x, ProbeSplit *out)
{
    uint32_t x0 = 0xFFFFu, x1 = 0u, y0 = 0xFFFFu, y1 = 0u;
    for (uint32_t i = 0; i < n; ++i) {
        const uint32_t y = tiles[i] / tiles_x, x = tiles[i] - y * tiles_x;
        if (x > 0xFFFFu || y > 0xFFFFu) return false;
        x0 = x < x0 ? x : x0; x1 = x > x1 ? x : x1;
        y0 = y < y0 ? y : y0; y1 = y > y1 ? y : y1;
    }
    out->x_range = x0 | x1 << 16;
    out->y_range = y0 | y1 << 16;
    return n != 0u;
}

// Which rows a launch renders: local row ly (0 <= ly < local_rows) is row
//   first_row + (ly / tile_rows) * tile_stride_rows + ly % tile_rows
// of the frame and row ly of the (packed) output buffer.
struct TileSpec {
    uint32_t first_row;
    uint32_t tile_rows;
    uint32_t tile_stride_rows;
    uint32_t local_rows;
};

// Device workspace of the streamed pipeline (primary_kernel / shadow_kernel / accumulate_kernel): the
// intermediate products that the fused kernel keeps in LDS live in HBM here.  Sized for the pixels of one
// launch (tiles x 64), grow-only, owned by the library per device.
struct TileDesc {
    uint32_t first;      // streamed pipeline: first hit record / result row block of the tile; probe pipeline: cost class
    uint32_t n_hit;
    uint32_t flags;      // bit 0: number the tile's rays sample-major; bit 1: queued for the reference re-render;
                         // bits 8-15: entries of the tile's cut (StreamWorkspace::cut)
    uint32_t pad;
};
struct HitRec {          // 48 B
    float p[3], n[3], rgb[3], pad[3];
};
static_assert(sizeof(TileDesc) == 16 && sizeof(HitRec) == 48, "stream record sizes");
// One entry of a tile's cut: the record range [begin, end) of the node stream that holds a subtree, and a copy of the
// subtree's ROOT record — a chunk tests the roots of its tile's cut out of LDS and fetches from the stream only below a
// root it passes.
struct CutEntry {
    uint32_t begin, end;
    NodeDev  root;
};
static_assert(sizeof(CutEntry) == 40, "CutEntry is ten dwords");
constexpr uint32_t kCutWords = sizeof(CutEntry) / 4u;
#ifndef RTX_MAX_CUT
#define RTX_MAX_CUT 16
#endif
constexpr uint32_t kMaxCut = RTX_MAX_CUT;
struct StreamWorkspace {
    HitRec   *hits;      // one per primary hit, compacted per tile
    uint32_t *pix_slot;  // tiles x 64: hit record of the pixel, or 0xFFFFFFFF
    TileDesc *tiles;     // one per tile
    uint2    *chunks;    // one per 64 shadow rays: (tile, chunk within the tile)
    float    *results;   // hits x nb_light: |n.l| or the "occluded" marker, per tile [sample][hit pixel]
    float    *acc;       // tiles x 64 x 3 running sums, only when nb_ray > 1
    uint32_t *ctr;       // hit count, chunk count, chunk cursor
    uint32_t *buckets;   // probe pipeline: tile order by cost class (layout: order_tiles_kernel)
    CutEntry *cut;       // tiles x kMaxCut entries (read by the ablation library; the whole-stream form keeps two words of answers in a tile's
                         // first entry), then — cut_stream_offset — tiles x kCutStreamRecords node records: the tiles' cuts
                         // as streams; written by probe_kernel, walked by shade_tiles_kernel
};
// Behind the tiles' CutEntry arrays, in the same buffer: every tile's cut once more AS A STREAM — kMaxCut node records of
// 32 bytes that the shading pass steps with the walk's own box step (rtx_traverse.hpp: walk_cut_stream): a real leaf's record
// as it is; for an inner root a record that LOOKS like a leaf (bit 31) with the root's box, link = the root's position in the
// node stream and info = kLeafFlag | kCutInnerFlag | the position behind its subtree.
// A tile's stream has kMaxCut + 1 records: the last one holds the box around ALL of the cut's roots (a chunk whose rays
// all miss it — most chunks that find no occluder — tests nothing else).
constexpr uint32_t kCutInnerFlag = 1u << 29, kCutEndMask = (1u << 26) - 1u;
constexpr uint32_t kCutStreamRecords = kMaxCut + 1u;
__host__ __device__ inline size_t cut_stream_offset(size_t tiles)      // bytes from StreamWorkspace::cut to the first stream
{
    return (tiles * kMaxCut * sizeof(CutEntry) + 63u) & ~static_cast<size_t>(63u);
}
struct StreamWorkspaceBytes { size_t hits, pix_slot, tiles, chunks, results, acc, ctr, buckets, cut; };
// Supported range of RTX_MAX_CUT.  Above: a job stages its tile's cut with ONE word per work-item of its 512
// (rtx_pass_shade.hpp: cut_word), so kCutWords * kMaxCut <= 512 — the build of round 2's cut-size sweep that printed no bench
// line (profiles/r02/h_ab_cut_size_with_roots_in_lds.log, "build 5" = 64 entries of the ten-word CutEntry = 640 words) left
// entries 51..63 of every cut unstaged and walked whatever LDS held; the same sweep before the roots moved into the
// entries (two words each, 128) had run.  Also <= 64: one wavefront holds the cut's frontier.  Below: an empty array.
static_assert(kMaxCut >= 1u && kMaxCut <= 51u && kCutWords * kMaxCut <= 512u, "RTX_MAX_CUT: 1 .. 51 (one staged word per work-item of 512)");
constexpr uint32_t kTileCutShift = 8u;       // TileDesc::flags
constexpr uint32_t kTileCompactHits = 8u;    // TileDesc::flags: the tile's hit records are in the compact form (rtx_pass_helpers.hpp: compact_hit_word)
constexpr uint32_t kTileChunk0Kept = 4u;     // TileDesc::flags: probe_kernel's probing walk answers the shading pass's chunk 0
StreamWorkspaceBytes stream_workspace_bytes(const DeviceScene &S, const TileSpec &ts, uint32_t variant);
constexpr uint32_t kCostBuckets = 64u;
constexpr uint32_t kStreamCtrWords = 4u;   // counters of the streamed (ablation) pipeline

// counters layout (uint64 x 8): 0 primary_hits, 1 box_tests, 2 tri_tests, 3 wave_node_visits, 4 wave_tri_visits,
// 5 tiles re-rendered by reference_tiles_kernel, 6 / 7 the part of 3 / 4 spent in probe_kernel (primary rays)
constexpr int kNumCounters = 8;

// Light samples per LDS batch (results of one batch: 64 pixels x batch floats): RTX_LIGHT_BATCH, scene_prep.h — the
// host orders each batch's walk.
// shade_tiles_kernel walks a batch's light samples along PreparedScene::light_tour, chunks dealt and drawn: the eight
// wavefronts of a workgroup walk neighbouring light points at the same time (results land in the sample's own column
// whatever the order, and the ordered accumulation reads the columns by ascending index).  The two other orders that
// were measured — the sample table's index order, and a contiguous run of the tour per wavefront — left the sources with
// their switch.

// Kernel variants, kept selectable (RTX_VARIANT) so that profiles can show what each choice is worth:
// bit 0 = conservative multiply-based box test for inner nodes (else the exact division-based one);
// bits 1-2 = wavefronts per workgroup of the fused kernel: 0 -> 4, 1 -> 8, 2 -> 2, 3 -> 1;
// bit 3 = streamed pipeline (three kernels, results through HBM) instead of the fused kernel.
// bit 4 (with bit 3) = two rays per lane in the shadow kernel, packed f32 arithmetic.
// bit 5 = probe pipeline: probe_kernel (primary hits of every tile + one probing shadow traversal that estimates the
// tile's cost) then shade_tiles_kernel (persistent workgroups, costliest tiles first, shadow + accumulation phases).
constexpr uint32_t kVariantStream = 8u;
constexpr uint32_t kVariantPacked = 16u;
constexpr uint32_t kVariantProbe = 32u;
constexpr uint32_t kVariantMask = 63u;
constexpr uint32_t kDefaultVariant = kVariantProbe | 1u;

// d_wave_prof: NULL or kWaveProfWords uint64 per 8x8 tile {node_visits, tri_visits, ~t_start, t_end, primary
// phase, slowest wave's shadow phase, accumulation phase, -} in ticks of the 100 MHz wall clock;
// zero-initialised by the caller, row-major over tiles with trace_tiles_x() tiles per row.
constexpr size_t kWaveProfWords = 8;
uint32_t trace_tiles_x(const DeviceScene &S, uint32_t variant);
// d_redo: the device work queue of a launch: [kQueueRedoCount] = number of tiles queued for the literal
// reference traversal, [kQueueNextTile] = next tile the persistent workgroups pull, tile ids from
// [kQueueHeader]; trace_redo_bytes() is its size for a launch.
// The two-pass pipeline keeps TWO such queues in the buffer, the second kQueueSlotStride words behind the first (its
// header in the first one's spare words), and launch n works on queue n & 1: no launch zeroes its own count — a launch
// zeroes the count of the NEXT one's queue, which nobody has read since the launch before (the invariant is written down
// at order_tiles_kernel).  The single-kernel forms use the first queue and zero its header themselves.
constexpr uint32_t kQueueRedoCount = 0u, kQueueNextTile = 1u, kQueueHeader = 4u, kQueueSlotStride = 2u;
size_t trace_redo_bytes(const DeviceScene &S, const TileSpec &ts);
// ws: workspace of the streamed / probe pipelines (may be NULL: the fused kernel is used then)
// phase_events: NULL or three events recorded on `stream`: launch start, end of the scheduling pass (probe + order;
// = start for the single-kernel variants), launch end (rtx_launch_timings)
// launch_no, pass_no (two-pass pipeline): how many launches, and how many primary-ray passes (nb_ray per launch), this
// d_redo and this workspace have served since their counting words were last zeroed (zero_launch_words) — by the caller, when
// either buffer is allocated or grown and after any other pipeline used them.  Their parities select the queue and the
// histogram a launch works on.
// split (two-pass pipeline): the scene's long list for launches that render the scene's own view of its uploaded geometry;
// the launcher drops it where probe_split_applies says no.
hipError_t launch_trace_shade(const DeviceScene &S, const TileSpec &ts, uint8_t *d_out, uint32_t *d_redo,
                              const StreamWorkspace *ws, unsigned long long *d_counters,
                              unsigned long long *d_wave_prof, uint32_t variant, hipStream_t stream,
                              hipEvent_t *phase_events = nullptr, uint32_t launch_no = 0u, uint32_t pass_no = 0u,
                              const ProbeSplit &split = ProbeSplit{nullptr, 0u, 0u, 0u});
// The same launch through the record forms of the kernels that store a pixel (rtx_kernel.hip, namespace rtxo): d_shade takes
// local_rows x width RtxPixelShade records, 16-byte aligned, one 16-byte store per pixel.  d_hits: trace_record_hits_bytes()
// bytes, the per-pixel hit counts a launch's passes hand on beside StreamWorkspace::acc (0: one ray per pixel, none needed —
// d_hits may be NULL).  The two-pass pipeline only, and never a long list.
hipError_t launch_trace_records(const DeviceScene &S, const TileSpec &ts, void *d_shade, uint8_t *d_hits, uint32_t *d_redo,
                                const StreamWorkspace *ws, unsigned long long *d_counters, uint32_t variant, hipStream_t stream,
                                hipEvent_t *phase_events = nullptr, uint32_t launch_no = 0u, uint32_t pass_no = 0u);
// The record launch behind the adaptive mean's tile mask (namespace rtxn: the scheduling pass's masked form): d_tiles holds an
// RtxTileState per 8 x 8 tile of the launch's rows, row by row, 8-byte aligned, written by an earlier launch on the stream; a
// tile that tile_stopped(rule, state) names is not scheduled and its records keep their words.  One band of rows (a view's
// launch), so that the launch's tile rows are the rectangle's.
hipError_t launch_trace_records_masked(const DeviceScene &S, const TileSpec &ts, void *d_shade, uint8_t *d_hits, uint32_t *d_redo,
                                       const StreamWorkspace *ws, unsigned long long *d_counters, uint32_t variant, hipStream_t stream,
                                       hipEvent_t *phase_events, uint32_t launch_no, uint32_t pass_no, const void *d_tiles,
                                       const RtxAdaptRule &rule);
size_t trace_record_hits_bytes(const DeviceScene &S, const TileSpec &ts);
// Whether a launch's tiles are tiles of the frame, so that the scene's long list names them: the share starts on a tile
// row, and every band of it but a single one is whole tile rows.  (Otherwise a tile of the launch straddles two of the frame.)
inline bool tiles_frame_aligned(const TileSpec &ts)
{
    return ts.first_row % 8u == 0u && ts.tile_stride_rows != 0u && ts.tile_rows != 0u &&
           ((ts.tile_rows % 8u == 0u && ts.tile_stride_rows % 8u == 0u) || ts.local_rows <= ts.tile_rows);
}
// Whether a launch is handed the scene's long list at all: the scene cuts per tile, the launch's tiles are the frame's, and
// the scheduling pass is bound by its longest wavefronts, not by throughput — up to kProbeSplitMaxTiles tiles, eight rounds
// of the device's 8,192 wavefront slots (a 4096 x 4096 frame's 262,144 tiles gain nothing from the list and paid +3.4 %
// of the pass for it: profiles/r08/e_ab_without_a_list.log).  Measured on either side of it: a 2560 x 1440 frame, 57,600
// tiles, gains (the pass 0.1003 ... 0.1011 -> 0.0941 ... 0.0946 ms); a 3840 x 2160 one, 129,600 tiles, would lose (0.1514 ...
// 0.1525 -> 0.1574 ... 0.1588); where between the two the sign changes is not measured (profiles/r08/h_ab_rectangle_gate_c5.log).
constexpr uint32_t kProbeSplitMaxTiles = 65536u;
inline bool probe_split_applies(const DeviceScene &S, const TileSpec &ts)
{
    const uint64_t tiles = static_cast<uint64_t>((S.width + 7u) / 8u) * ((ts.local_rows + 7u) / 8u);
    return S.n_nodes <= S.cut_max_nodes && ts.local_rows != 0u && tiles_frame_aligned(ts) && tiles <= kProbeSplitMaxTiles;
}
// zeroes those counting words (both queues' headers, the workspace's order words in front of its job list) on `stream`
hipError_t zero_launch_words(uint32_t *d_redo, const StreamWorkspace &ws, hipStream_t stream);

}  // namespace rtx
