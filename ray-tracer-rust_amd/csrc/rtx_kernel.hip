// rtx_kernel.hip — the per-pixel tracer for gfx950 (MI355X, CDNA4): kernels and launcher.
//
// Replaces render_pixel() + everything below it in the reference
// (src/main.rs:151-240, src/tracer/**); citations are path:line in that repository.
// The traversal itself is in rtx_traverse.hpp; the passes of a launch are in rtx_pass_helpers.hpp (tile and pixel helpers),
// rtx_pass_schedule.hpp (probe_kernel), rtx_pass_order.hpp (the counting and ordering kernels) and rtx_pass_shade.hpp
// (shade_tiles_kernel), the timing instrumentation of tools/ in rtx_probes.hpp.  This file: reference_tiles_kernel, the
// record forms of the three kernels that store a pixel (namespace rtxo; they share the byte forms'
// bodies), the masked form of the scheduling pass (namespace rtxn: the record form behind the adaptive mean's tile mask), the
// launcher, and the text that says what the library was built with.
//
// A launch (launch_probe, further down) is two passes over the 8x8-pixel tiles of its rows, four dispatches:
//   scheduling pass   probe_kernel (one wavefront per tile, one work-item per pixel: primary ray, closest hit,
//                     compacted hit records to HBM, one probing shadow walk = the tile's cost estimate, counted in
//                     a sharded histogram), order_tiles_kernel (counting sort of the tiles by cost class; it also
//                     zeroes the words the next pass and the next launch count in);
//   shading pass      shade_tiles_kernel — persistent workgroups of 8 wavefronts pull jobs (tiles or parts of
//                     tiles) costliest first.  Per job: one work-item per SHADOW RAY — the (hit pixel, light sample)
//                     pairs are dealt to the wavefronts in chunks of 64 consecutive rays, a thin shaft towards the
//                     small area light, which is what makes the wave-uniform walk cheap; each ray stores |n.l|
//                     (lit) or a marker (occluded) in LDS — then one work-item per PIXEL adds the samples in
//                     sample order, exactly the reference's sequential f32 accumulation (main.rs:209-216),
//                     quantises and stores RGB8.
//   reference_tiles_kernel — the rare tiles in which some ray has a -0.0 / non-finite direction component (the
//                     regime where the reference's result depends on its own tree) are queued by either pass and
//                     re-rendered here, one work-item per pixel, with the literal reference traversal.  It reads
//                     the queue length on the device, so an empty queue costs one kernel boundary.
//
// librtx.so holds these four kernels and two small ones off the frame's path: reset_kernel (the counting words of a new
// or grown workspace, once) and count_classes_kernel (the whole-stream form's histogram).  The earlier forms of the pipeline (a fused single kernel,
// a streamed three-kernel pipeline, two rays per lane) live in rtx_ablation_kernels.hpp and are compiled only into
// librtx_ablation.so (-DRTX_ABLATION=1), where RTX_VARIANT selects them for A/B runs and the variant-equality test.
//
// The gamma curve is not evaluated on the device: scene_prep locates the 255 byte steps of
// (x.powf(1/2.2)*255) as u8 with the host libm and the kernels count thresholds <= x.
#include <cstdlib>
#include <type_traits>
#if defined(RTX_RECORD_FORMS) || defined(RTX_MASKED_FORMS)
#error "RTX_RECORD_FORMS and RTX_MASKED_FORMS are not build switches: this file sets them around its further inclusions of the passes' headers"
#endif
#include "rtx_traverse.hpp"
// the passes, one file each (a kernel of a later one uses what the earlier ones define; one translation unit)
#include "rtx_pass_helpers.hpp"
#include "rtx_pass_schedule.hpp"
#include "rtx_pass_order.hpp"
#include "rtx_pass_shade.hpp"

namespace rtx {

// One wavefront per queued tile, one work-item per pixel, the reference's loop order (main.rs:180-240)
// with the literal reference traversal.  Slow by construction (the reference's tree visits thousands of
// boxes per ray); only tiles holding a zero-component ray come here.
template <bool COUNT, bool SPHERES = false>
__global__ void __launch_bounds__(64) reference_tiles_kernel(DeviceScene S, TileSpec ts, uint32_t tiles_x,
                                                              uint8_t *__restrict__ out,
                                                              const uint32_t *__restrict__ redo,
                                                              unsigned long long *__restrict__ counters,
                                                              bool tile_blocks = false)
{
#include "rtx_reference_body.inc"
}

}  // namespace rtx

// The record forms of the three kernels that store a pixel (rtx_render_view_rows_shade): the same bodies (the two passes'
// headers included a second time, rtx_reference_body.inc) with a RecordOut —
// one 16-byte store per pixel in place of three byte stores.  A namespace of their own: the byte forms keep their symbols.
// Only the forms a view's launch is handed: probe_kernel's one-wavefront form (a view's launch has no long list).
namespace rtxo {

using namespace rtx;

#define RTX_RECORD_FORMS 1      // probe_records_kernel and shade_records_kernel: the two headers' kernels once more
#include "rtx_pass_schedule.hpp"
#include "rtx_pass_shade.hpp"
#undef RTX_RECORD_FORMS

template <bool COUNT, bool SPHERES>
__global__ void __launch_bounds__(64) reference_records_kernel(DeviceScene S, TileSpec ts, uint32_t tiles_x,
                                                                uint4 *__restrict__ out_shade,
                                                                const uint32_t *__restrict__ redo,
                                                                unsigned long long *__restrict__ counters)
{
    constexpr bool tile_blocks = true;
    const RecordOut out{out_shade, nullptr};
#include "rtx_reference_body.inc"
}

}  // namespace rtxo

// The masked form of the scheduling pass (rtx_render_view_rows_adaptive, rtx_render_view_rows_shade_masked_device):
// probe_records_kernel's text a third time, behind the adaptive mean's tile mask — a stopped tile is not scheduled, so the
// shading pass and the reference pass are rtxo's, unchanged.  A top-level namespace of its own: every other kernel set keeps
// its symbols.
namespace rtxn {

using namespace rtx;

#define RTX_RECORD_FORMS 1
#define RTX_MASKED_FORMS 1      // probe_masked_kernel
#include "rtx_pass_schedule.hpp"
#undef RTX_MASKED_FORMS
#undef RTX_RECORD_FORMS

}  // namespace rtxn

namespace rtx {


namespace {

// kSplitShare: a tile whose estimated cost is above this fraction of a workgroup's fair share of the launch is split
// (the ablation build reads RTX_SPLIT_SHARE once instead: tools/share_timing.py sweeps it)
// (50 until the estimates learned to tell the tiles apart — the probing walk of cut tiles, mixed tiles twice; with them
//  a whole fair share: big_bunny 1080p 0.855 -> 0.825 ms over five interleaved rounds, one share of 4 / 8 -1.3 / -0.4 %,
//  of 2 +0.8 %; profiles/r03/xh_ab_split_share.log.  Round 6 gave half a share its six rounds: alone, big_bunny 1080p
//  0.7585 ... 0.7655 against 0.7714 ... 0.7864, everything else +0.1 ... 0.3 %; TOGETHER with the raised share by launch
//  size, which is worth as much there and costs less elsewhere, the small bunny's frame +4 % (0.2802 ... 0.2818 against
//  0.2688 ... 0.2694): a whole share stays; profiles/r07/b_ab_piece4.log, c_ab_piece4_combined.log)
#ifndef RTX_SPLIT_SHARE_PERCENT
#define RTX_SPLIT_SHARE_PERCENT 100
#endif
constexpr float kSplitShare = RTX_SPLIT_SHARE_PERCENT * 0.01f;
float split_share()
{
#if RTX_ABLATION
    static const float v = [] {
        const char *e = getenv("RTX_SPLIT_SHARE");
        const float x = e ? strtof(e, nullptr) : 0.0f;
        return x > 0.0f ? x : kSplitShare;
    }();
    return v;
#else
    return kSplitShare;
#endif
}

// The record output behind the adaptive mean's tile mask: rtxn::probe_masked_kernel's three further arguments
struct MaskedOut {
    RecordOut records;
    const RtxTileState *tiles;       // one per 8 x 8 tile of the rectangle, row by row; 8-byte aligned
    uint32_t min_frames;
    float max_variance;
};
inline uint8_t *records_of(uint8_t *out) { return out; }
inline RecordOut records_of(const RecordOut &out) { return out; }
inline RecordOut records_of(const MaskedOut &out) { return out.records; }

// OUT: uint8_t * (the byte forms), RecordOut (the record forms, rtxo) or MaskedOut (the record forms, their scheduling pass
// masked: rtxn)
template <bool COUNT, bool FAST, bool SPHERES, class OUT>
hipError_t launch_probe(const DeviceScene &S, const TileSpec &ts, OUT d_out, uint32_t *d_redo,
                        const StreamWorkspace &W, unsigned long long *d_counters, hipStream_t stream, hipEvent_t *ev,
                        uint32_t launch_no, uint32_t pass_no, const ProbeSplit &split_in)
{
#ifndef RTX_SHADE_NW
#define RTX_SHADE_NW 8
#endif
    constexpr int NW = RTX_SHADE_NW;     // wavefronts per workgroup of shade_tiles_kernel
    // the form of the two kernels that have two: per-tile cuts, or — a scene too large for them — the whole stream
    const bool whole = S.n_nodes > S.cut_max_nodes;
    constexpr bool kMasked = std::is_same<OUT, MaskedOut>::value;
    constexpr bool kRecords = std::is_same<OUT, RecordOut>::value || kMasked;
    const auto d_rec = records_of(d_out);     // (the byte forms: d_out itself)
    const auto shade_bytes = whole ? shade_tiles_kernel<COUNT, FAST, NW, SPHERES, true> : shade_tiles_kernel<COUNT, FAST, NW, SPHERES, false>;
    const auto shade_records = whole ? rtxo::shade_records_kernel<COUNT, FAST, NW, SPHERES, true> : rtxo::shade_records_kernel<COUNT, FAST, NW, SPHERES, false>;
    const uint32_t batch = S.nb_light < kMaxLightBatch ? (S.nb_light ? S.nb_light : 1u) : kMaxLightBatch;
#if RTX_ABLATION
    const size_t lds_bytes = (static_cast<size_t>(lds_floats(batch)) + (S.j1_mode == 1u ? kJ1WindowWords : 0u)) * sizeof(float);
#else
    const size_t lds_bytes = static_cast<size_t>(lds_floats(batch)) * sizeof(float);
#endif
    const uint32_t tiles_x = (S.width + 7u) / 8u, tiles_y = (ts.local_rows + 7u) / 8u;
    const uint32_t n_tiles = numbered_tiles(tiles_x, tiles_y);
    // The long list, where it applies (rtx_device.h: probe_split_applies).  With a list: its workgroups first, padded to whole
    // rounds of the XCDs, then one workgroup per four tiles.  Without: one workgroup per tile, in whole runs of 64 tile numbers
    // over the 8 XCDs.
    const ProbeSplit split = (split_in.n_long != 0u && split_in.words && probe_split_applies(S, ts)) ? split_in : ProbeSplit{nullptr, 0u, 0u, 0u};
    const uint32_t probe_waves = split.n_long != 0u ? 4u : 1u;
    const uint32_t probe_grid = split.n_long != 0u ? ((split.n_long + 7u) & ~7u) + 128u * ((n_tiles + 511u) / 512u) : 512u * ((n_tiles + 511u) / 512u);
    if (kRecords && split.n_long != 0u) return hipErrorInvalidValue;     // (the record forms have no four-beam probe_kernel)
    if constexpr (kMasked)
        if (!d_out.tiles || (reinterpret_cast<uintptr_t>(d_out.tiles) & 7u)) return hipErrorInvalidValue;
    const auto probe = whole ? probe_kernel<COUNT, FAST, SPHERES, true, 1u>
                     : split.n_long != 0u ? probe_kernel<COUNT, FAST, SPHERES, false, 4u> : probe_kernel<COUNT, FAST, SPHERES, false, 1u>;
    const auto probe_records = whole ? rtxo::probe_records_kernel<COUNT, FAST, SPHERES, true> : rtxo::probe_records_kernel<COUNT, FAST, SPHERES, false>;
    const auto probe_masked = whole ? rtxn::probe_masked_kernel<COUNT, FAST, SPHERES, true> : rtxn::probe_masked_kernel<COUNT, FAST, SPHERES, false>;
    // persistent grid = what the device keeps resident of the form that is launched (the cut and whole-stream forms differ in
    // registers, and so may the byte and record forms: each instantiation of this launcher — one per OUT — has its own cache)
    static thread_local int cached_dev = -1, cached_blocks = 0;
    static thread_local size_t cached_lds = 0;
    static thread_local bool cached_whole = false;
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    if (dev != cached_dev || lds_bytes != cached_lds || whole != cached_whole) {
        int per_cu = 0, cus = 0;
        if (kRecords) e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, shade_records, 64 * NW, lds_bytes);
        else e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, shade_bytes, 64 * NW, lds_bytes);
        if (e != hipSuccess) return e;
        if ((e = hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev)) != hipSuccess) return e;
        cached_blocks = (per_cu > 0 ? per_cu : 1) * (cus > 0 ? cus : 1);
        cached_dev = dev;
        cached_lds = lds_bytes;
        cached_whole = whole;
    }
    if (n_tiles > kJobTileMask) return hipErrorInvalidValue;
    const uint64_t most_jobs = (uint64_t)n_tiles * kMaxTileParts;
    const uint32_t grid = most_jobs < static_cast<uint64_t>(cached_blocks) ? (uint32_t)most_jobs : static_cast<uint32_t>(cached_blocks);
    uint32_t *const queue = d_redo + (launch_no & 1u) * kQueueSlotStride;            // rtx_device.h: two queues, taken in turn
    uint32_t *const next_redo_count = d_redo + ((launch_no + 1u) & 1u) * kQueueSlotStride + kQueueRedoCount;
    for (uint32_t r = 0; r < S.nb_ray; ++r) {                                        // main.rs:186
        // four dispatches a pass, five in the whole-stream form: no kernel only zeroes, and only the whole-stream form has
        // one that only counts (the table in front of kOrderList)
        const uint32_t hist_set = (pass_no + r) & 1u;
        const StreamWorkspace Wp = counting_set(W, hist_set);      // what the kernels that count are handed
        if constexpr (kMasked)
            hipLaunchKernelGGL(probe_masked, dim3(probe_grid), dim3(64), 0, stream,
                               S, ts, tiles_x, n_tiles, r, Wp, d_rec.shade, d_rec.hits, queue, d_counters, d_out.tiles, d_out.min_frames,
                               d_out.max_variance);
        else if constexpr (kRecords)
            hipLaunchKernelGGL(probe_records, dim3(probe_grid), dim3(64), 0, stream,
                               S, ts, tiles_x, n_tiles, r, Wp, d_rec.shade, d_rec.hits, queue, d_counters);
        else
            hipLaunchKernelGGL(probe, dim3(probe_grid), dim3(64 * probe_waves), 0, stream,
                               S, ts, tiles_x, n_tiles, r, Wp, d_out, queue, d_counters, split);
        if (whole) hipLaunchKernelGGL(count_classes_kernel, dim3((n_tiles + 1023u) / 1024u), dim3(1024), 0, stream, n_tiles, Wp);
        hipLaunchKernelGGL(order_tiles_kernel, dim3((n_tiles + 1023u) / 1024u), dim3(1024), 0, stream, n_tiles, W, grid, split_share(),
                           hist_set, whole ? 0u : grid, queue, next_redo_count);
        if (ev && r == 0u && (e = hipEventRecord(ev[1], stream)) != hipSuccess) return e;   // end of the scheduling pass
        if constexpr (kRecords)
            hipLaunchKernelGGL(shade_records, dim3(grid), dim3(64 * NW), lds_bytes, stream, S, ts, batch, tiles_x, n_tiles, r, W,
                               d_rec.shade, d_rec.hits, queue, d_counters);
        else
            hipLaunchKernelGGL(shade_bytes, dim3(grid), dim3(64 * NW), lds_bytes, stream, S, ts, batch, tiles_x, n_tiles, r, W, d_out, queue, d_counters);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    if constexpr (kRecords)
        hipLaunchKernelGGL((rtxo::reference_records_kernel<COUNT, SPHERES>), dim3(n_tiles < 1024u ? n_tiles : 1024u), dim3(64), 0, stream,
                           S, ts, tiles_x, d_rec.shade, queue, d_counters);
    else
        hipLaunchKernelGGL((reference_tiles_kernel<COUNT, SPHERES>), dim3(n_tiles < 1024u ? n_tiles : 1024u), dim3(64), 0, stream,
                           S, ts, tiles_x, d_out, queue, d_counters, true);
    return hipGetLastError();
}

}  // namespace

#if RTX_ABLATION
#include "rtx_ablation_kernels.hpp"
#endif

// (every kernel form has the same tiles per row: the variant decides nothing here and stays in the exported signature)
uint32_t trace_tiles_x(const DeviceScene &S, uint32_t) { return (S.width + 7u) / 8u; }

hipError_t zero_launch_words(uint32_t *d_redo, const StreamWorkspace &W, hipStream_t stream)
{
    hipLaunchKernelGGL(reset_kernel, dim3(1), dim3(256), 0, stream, d_redo, 0u, kQueueSlotStride + kQueueHeader, W.buckets, kOrderList);
    return hipGetLastError();
}

size_t trace_redo_bytes(const DeviceScene &S, const TileSpec &ts)
{
    return sizeof(uint32_t) * (kQueueSlotStride + kQueueHeader + static_cast<size_t>(numbered_tiles((S.width + 7u) / 8u, (ts.local_rows + 7u) / 8u)));
}

StreamWorkspaceBytes stream_workspace_bytes(const DeviceScene &S, const TileSpec &ts, uint32_t variant)
{
    const bool streamed = (variant & kVariantStream) != 0u, probe = (variant & kVariantProbe) != 0u;
    const size_t tiles = probe ? numbered_tiles((S.width + 7u) / 8u, (ts.local_rows + 7u) / 8u)
                               : static_cast<size_t>((S.width + 7u) / 8u) * ((ts.local_rows + 7u) / 8u);
    const size_t pixels = tiles * 64u;
    StreamWorkspaceBytes b;
    b.hits = pixels * sizeof(HitRec);
    b.pix_slot = pixels * sizeof(uint32_t);
    b.tiles = tiles * sizeof(TileDesc);
    b.chunks = streamed ? (pixels * S.nb_light / 64u + tiles + 1u) * sizeof(uint2) : 0u;
    b.results = streamed ? pixels * (S.nb_light ? S.nb_light : 1u) * sizeof(float) : 0u;
    b.acc = S.nb_ray > 1u ? pixels * 3u * sizeof(float) : 0u;
    b.ctr = kStreamCtrWords * sizeof(uint32_t);   // streamed (ablation) pipeline only; 16 B
    b.buckets = probe ? (kOrderList + tiles * kMaxTileParts) * sizeof(uint32_t) : 0u;
    b.cut = probe ? cut_stream_offset(tiles) + tiles * kCutStreamRecords * sizeof(NodeDev) : 0u;     // CutEntry arrays, then the cut streams
    return b;
}

template <class OUT>
static hipError_t launch_dispatch(const DeviceScene &S, const TileSpec &ts, OUT d_out, uint32_t *d_redo,
                                  const StreamWorkspace *ws, unsigned long long *d_counters,
                                  unsigned long long *d_wave_prof, uint32_t variant, hipStream_t stream, hipEvent_t *ev,
                                  uint32_t launch_no, uint32_t pass_no, const ProbeSplit &split)
{
    // the two-pass pipeline: launch_probe<COUNT, FAST, SPHERES, OUT> for the caller's counters and the scene's primitives
    auto two_pass = [&](auto fast) {
        constexpr bool FAST = decltype(fast)::value;
        const bool count = d_counters != nullptr, spheres = S.n_spheres != 0u;
        const auto launch = count ? (spheres ? launch_probe<true, FAST, true, OUT> : launch_probe<true, FAST, false, OUT>)
                                  : (spheres ? launch_probe<false, FAST, true, OUT> : launch_probe<false, FAST, false, OUT>);
        return launch(S, ts, d_out, d_redo, *ws, d_counters, stream, ev, launch_no, pass_no, split);
    };
#if RTX_ABLATION
    if (!((variant & kVariantProbe) && ws && !d_wave_prof)) {
        if constexpr (!std::is_same<OUT, uint8_t *>::value) return hipErrorInvalidValue;   // (records: the two-pass pipeline's alone)
        else return launch_dispatch_ablation(S, ts, d_out, d_redo, ws, d_counters, d_wave_prof, variant, stream);
    }
    if (!(variant & 1u)) return two_pass(std::false_type{});   // with the exact (division-based) box test on inner nodes
#else
    if (variant != kDefaultVariant || !ws || d_wave_prof) return hipErrorInvalidValue;   // one pipeline in this build
#endif
    return two_pass(std::true_type{});
}

template <class OUT>
static hipError_t launch_any(const DeviceScene &S, const TileSpec &ts, OUT d_out, uint32_t *d_redo,
                             const StreamWorkspace *ws, unsigned long long *d_counters,
                             unsigned long long *d_wave_prof, uint32_t variant, hipStream_t stream,
                             hipEvent_t *phase_events, uint32_t launch_no, uint32_t pass_no, const ProbeSplit &split)
{
    if (ts.local_rows == 0) return hipSuccess;
    hipError_t e;
    if (phase_events && (e = hipEventRecord(phase_events[0], stream)) != hipSuccess) return e;
    const bool probe = (variant & kVariantProbe) && ws && !d_wave_prof;
    if (phase_events && !probe && (e = hipEventRecord(phase_events[1], stream)) != hipSuccess) return e;
    e = launch_dispatch(S, ts, d_out, d_redo, ws, d_counters, d_wave_prof, variant, stream, probe ? phase_events : nullptr, launch_no, pass_no, split);
    if (e != hipSuccess) return e;
    if (phase_events && (e = hipEventRecord(phase_events[2], stream)) != hipSuccess) return e;
    return hipSuccess;
}

hipError_t launch_trace_shade(const DeviceScene &S, const TileSpec &ts, uint8_t *d_out, uint32_t *d_redo,
                              const StreamWorkspace *ws, unsigned long long *d_counters,
                              unsigned long long *d_wave_prof, uint32_t variant, hipStream_t stream,
                              hipEvent_t *phase_events, uint32_t launch_no, uint32_t pass_no, const ProbeSplit &split)
{
    return launch_any(S, ts, d_out, d_redo, ws, d_counters, d_wave_prof, variant, stream, phase_events, launch_no, pass_no, split);
}

hipError_t launch_trace_records(const DeviceScene &S, const TileSpec &ts, void *d_shade, uint8_t *d_hits, uint32_t *d_redo,
                                const StreamWorkspace *ws, unsigned long long *d_counters, uint32_t variant, hipStream_t stream,
                                hipEvent_t *phase_events, uint32_t launch_no, uint32_t pass_no)
{
    if (!ws || !d_shade || (S.nb_ray > 1u && !d_hits)) return hipErrorInvalidValue;
    return launch_any(S, ts, RecordOut{static_cast<uint4 *>(d_shade), d_hits}, d_redo, ws, d_counters, nullptr, variant, stream,
                      phase_events, launch_no, pass_no, ProbeSplit{nullptr, 0u, 0u, 0u});
}

hipError_t launch_trace_records_masked(const DeviceScene &S, const TileSpec &ts, void *d_shade, uint8_t *d_hits, uint32_t *d_redo,
                                       const StreamWorkspace *ws, unsigned long long *d_counters, uint32_t variant, hipStream_t stream,
                                       hipEvent_t *phase_events, uint32_t launch_no, uint32_t pass_no, const void *d_tiles,
                                       const RtxAdaptRule &rule)
{
    if (!ws || !d_shade || (S.nb_ray > 1u && !d_hits) || !d_tiles || (reinterpret_cast<uintptr_t>(d_tiles) & 7u)) return hipErrorInvalidValue;
    if (ts.first_row + ts.local_rows > S.height || ts.tile_rows != ts.local_rows) return hipErrorInvalidValue;   // one band: a view's rows
    const MaskedOut out{RecordOut{static_cast<uint4 *>(d_shade), d_hits}, static_cast<const RtxTileState *>(d_tiles), rule.min_frames,
                        rule.max_variance};
    return launch_any(S, ts, out, d_redo, ws, d_counters, nullptr, variant, stream, phase_events, launch_no, pass_no,
                      ProbeSplit{nullptr, 0u, 0u, 0u});
}

size_t trace_record_hits_bytes(const DeviceScene &S, const TileSpec &ts)
{
    return S.nb_ray > 1u ? static_cast<size_t>(numbered_tiles((S.width + 7u) / 8u, (ts.local_rows + 7u) / 8u)) * 64u : 0u;
}

}  // namespace rtx

// What this library was built with: every compile-time switch of the kernel sources and its value, as text in the
// binary.  tests/test_host_prep.py compares the string in the shipped librtx.so with the one a preprocessor run without
// any -D produces, and checks that no switch of the sources is missing here: an A/B build cannot be mistaken for the
// product.  (The timing instrumentation switches count as well: they cost time.  RTX_WAVES_PER_SIMD and
// RTX_PACKED_WAVES_PER_SIMD belong to rtx_ablation_kernels.hpp: the product does not include it, nothing in it reads them,
// and its text gives each its own name for a value — unless a -D set one.)
#define RTX_SW_STR2(x) #x
#define RTX_SW_STR(x) RTX_SW_STR2(x)
#define RTX_SW(x) " " #x "=" RTX_SW_STR(x)
extern "C" __attribute__((used, visibility("hidden"))) const char rtx_build_switches_text[] = "rtx-build-switches:"
    RTX_SW(RTX_CLAIM_RUN_LOG) RTX_SW(RTX_CUT_DRAW_MIN) RTX_SW(RTX_CUT_UNION_MIN) RTX_SW(RTX_LIGHT_BATCH) RTX_SW(RTX_MAX_CUT)
    RTX_SW(RTX_PACKED_WAVES_PER_SIMD) RTX_SW(RTX_PROBE_LONG_WEIGHT) RTX_SW(RTX_PROBE_VISIT_SCALE) RTX_SW(RTX_PROBE_WAVES_PER_SIMD)
    RTX_SW(RTX_SHADE_CUT_WAVES_PER_SIMD) RTX_SW(RTX_SHADE_NW) RTX_SW(RTX_SHADE_WAVES_PER_SIMD)
    RTX_SW(RTX_SPLIT_SHARE_PERCENT) RTX_SW(RTX_TILE_PARTS_MAX) RTX_SW(RTX_WAVES_PER_SIMD)
    RTX_SW(RTX_EXPERIMENT_TIMELINE) RTX_SW(RTX_EXPERIMENT_PHASES) RTX_SW(RTX_EXPERIMENT_PROBE_PHASES) RTX_SW(RTX_ABLATION);
#undef RTX_SW
