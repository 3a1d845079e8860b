// rtx_pass_schedule.hpp — the render pipeline's scheduling pass (rtx_kernel.hip): probe_kernel, one wavefront per tile —
// primary rays, hit records, the tile's cut (its shaft against the tree) and its cost estimate — with what it is made of.
// The tiles the scene predicts long (ProbeSplit) start first, a workgroup each, their primary rays walked as four beams.
//
// rtx_kernel.hip includes this file a second time, inside namespace rtxo with RTX_RECORD_FORMS defined: then probe_kernel's text
// alone is compiled once more, as rtxo::probe_records_kernel — the same body with `out` a RecordOut (rtx_pass_helpers.hpp) and
// one wavefront per tile (a view's launch has no long list).  The sky store is the one statement that differs, through
// store_pixel's overloads.  (Why text compiled twice and not a __device__ template: rtx_pass_shade.hpp.)
//
// ... and a third time, inside namespace rtxn with RTX_MASKED_FORMS defined beside RTX_RECORD_FORMS: the record form behind the
// adaptive mean's tile mask, rtxn::probe_masked_kernel.  Once the wavefront knows its tile it reads the tile's 8-byte state
// (RtxTileState, numbered row by row over the rectangle: NOT tile_id, which is swizzled), makes the two words scalars and
// evaluates scene_prep.h's tile_stopped: a stopped tile gets a descriptor that schedules nothing and the wavefront returns;
// a live tile runs the record form's body, token for token.
#if !defined(RTX_PASS_SCHEDULE_HPP) || defined(RTX_RECORD_FORMS)
#if !defined(RTX_RECORD_FORMS)
#define RTX_PASS_SCHEDULE_HPP
#include "rtx_probes.hpp"
#include "rtx_pass_helpers.hpp"

namespace rtx {

// =====================================================================================================
// Probe pipeline: the fused kernel with its first phase moved out, so that tiles can be scheduled by cost.
// A frame's tiles differ in cost by three orders of magnitude (sky: nothing; ground: ~13 records per shadow
// walk; mesh silhouettes and the shadow: hundreds), and a persistent workgroup that pulls a costly tile late
// holds the frame's tail alone (profiles/r01: the last 1 % of the tiles end 10 % after the rest).
//
//   probe_kernel        one wavefront per tile: primary rays, closest hits, compacted hit records to HBM
//                       (64 x 48 B per tile, read back once) — and ONE shadow walk, the tile's hit pixels towards
//                       light sample 0, whose record count times the tile's number of 64-ray chunks is the cost
//                       estimate.  The tile id is appended to the list of its cost class (half octaves).
//   shade_tiles_kernel  persistent workgroups pull tiles costliest class first; phases 2 and 3 of the fused kernel.
//
// Same arithmetic, same order of additions, same bytes as trace_shade_kernel.
__device__ __forceinline__ uint32_t cost_class(unsigned long long cost)
{
    if (cost == 0ull) return 0u;
    if (cost > 0x7FFFFFFFull) cost = 0x7FFFFFFFull;
    const uint32_t c = (uint32_t)cost;
    const uint32_t lz = 31u - (uint32_t)__clz((int)c);                 // floor(log2)
    const uint32_t half = lz ? (c >> (lz - 1u)) & 1u : 0u;
    const uint32_t k = 2u * lz + half + 1u;
    return k < kCostBuckets ? k : kCostBuckets - 1u;
}

// what a chunk costs before it fetches its first record (ray set-up, the global triangles, its share of the ordered sum),
// in units of one fetched record: the weight of a tile whose cut is empty
constexpr uint32_t kChunkFixedCost = 8u;


// Cut form: a tile whose cut has at least this many entries — a tile that walks — draws its chunks as well (0: none do).
// Round 2 measured this a loss (+1 % on big_bunny 1080p: the walks were slower then and the jobs that never draw paid for
// the loop's shape); with the hand-written box step it is -2.3 % there (six interleaved rounds) and -0.5 % at 4096x4096;
// from 8 entries on: -2.1 % / -0.3 % (profiles/r03/x4_*).
#ifndef RTX_CUT_DRAW_MIN
#define RTX_CUT_DRAW_MIN 1
#endif
// the entry form of a tile's cut (CutEntry, staged in LDS by a job) is read by the ablation library's variants only
constexpr bool kCutEntriesUsed = RTX_ABLATION != 0;
// wavefronts per workgroup of probe_kernel, its template parameter WAVES.  1: one tile per workgroup, the form of every
// launch without a long list.  4: a launch with a long list — four independent tiles, or the four beams of one long tile.
// (Four tiles per workgroup alone measured the same in round 2, j_ab_probe_tiles_per_workgroup.log; in round 7 it is +1.3 %
// on the pass of a 4096 x 4096 frame, profiles/r08/e_ab_without_a_list.log: only the launches that gain from the list pay it.)
// Wavefronts per SIMD probe_kernel's register allocation must allow: a 4096 x 4096 frame's 262,144 one-wavefront workgroups
// are bound by how many of them are resident (the probing walk of cut tiles brought the kernel to 106 scalar registers: 7)
#ifndef RTX_PROBE_WAVES_PER_SIMD
#define RTX_PROBE_WAVES_PER_SIMD 8
#endif
#ifndef RTX_PROBE_VISIT_SCALE         // a record of the probing walk of a cut tile (probe_cut_walk) in the units of the cut's proxy
#define RTX_PROBE_VISIT_SCALE 6u
#endif

// ---- the cut of a tile ------------------------------------------------------------------------------------------
// The hundred chunks of a tile send their shadow rays from its hit points to the same few light points: all of them
// lie in the SHAFT between O, the bounding box of the tile's hit points, and L, the bounding box of the light points
// — the convex hull of O and L, which for axis-aligned boxes is the union over s in [0, 1] of the boxes whose bounds
// run linearly from O's to L's ((1-s) O + s L, a Minkowski combination of boxes, is the box with the interpolated
// bounds).  A node's box B meets the shaft iff some s satisfies six inequalities that are linear in s:
//     B.lo_a <= O.hi_a + s (L.hi_a - O.hi_a)        B.hi_a >= O.lo_a + s (L.lo_a - O.lo_a)        a = x, y, z
// — one division each, the same shape as a ray's slab test.  probe_kernel descends the tree ONCE per tile with this
// test, breadth first, one node per work-item, and leaves the CUT in HBM: the subtrees (leaves, mostly) whose boxes
// meet the shaft.  shade_tiles_kernel's chunks then walk these and nothing else (rtx_traverse.hpp: walk_cut): the
// upper levels of the tree are descended once per tile instead of once per chunk, and the tiles whose shaft meets no
// leaf — most of the open ground — do not walk at all.
//
// Soundness: culling only has to keep a superset.  A ray of the tile runs from a hit point p in O towards a light
// point l in L; a candidate that can occlude it lies at a distance of at most the light's (main.rs:219-231, any-hit:
// rtx_traverse.hpp), i.e. on the segment p..l, which the hull contains.  What the hull is compared with are the
// reference's FLOATING-POINT box tests on a direction that is itself rounded: a box the reference accepts is met by
// the true segment within a few units in the last place of the scene's largest coordinate M (the quotients of
// bounding_box.rs:120-157 carry two roundings each, the unit direction three: below 2^-20 M in position units
// together).  The test therefore takes every box DELTA = 2^-16 M larger on every side
// (PreparedScene::shaft_delta; the stream's boxes are already 2^-19 M larger, cull_delta) and lets s run over
// [-2^-8, 1 + 2^-8]; the same margin covers its own roundings (one reciprocal, one fused multiply-add per plane:
// 2^-22 M in position units).  An inequality whose slope is zero or tiny is dropped, which only enlarges the
// superset.  Nothing here decides a pixel: the rays still test every box and triangle of the cut themselves.
struct Shaft {
    float inv[6], off[6];     // q_c = plane_c * inv[c] + off[c]: the s at which constraint c becomes tight
    uint32_t lower, upper;    // bit c: q_c is a lower / an upper bound of s (neither: the constraint is dropped)
};
constexpr float kShaftS0 = -0x1p-8f, kShaftS1 = 1.0f + 0x1p-8f;

// constraint c = 2a (lower plane of B on axis a against the upper bound of the interpolated box) or 2a+1 (upper plane
// against its lower bound); o = O's corner, g = L's corner - O's corner on that side
__device__ __forceinline__ void shaft_constraint(Shaft &sh, uint32_t c, float o, float g, float delta)
{
    // c even:  B.lo - delta - o <= s g      g > 0: s >= q (lower bound)    g < 0: s <= q (upper bound)
    // c odd:   B.hi + delta - o >= s g      g > 0: s <= q (upper bound)    g < 0: s >= q (lower bound)
    const bool usable = fabsf(g) >= 0x1p-40f && fabsf(g) <= 0x1p60f;      // else dropped (conservative)
    const float inv = __builtin_amdgcn_rcpf(g);
    sh.inv[c] = usable ? inv : 0.0f;
    sh.off[c] = usable ? (((c & 1u) ? delta : -delta) - o) * inv : 0.0f;
    const bool positive = g > 0.0f;
    const bool is_lower = usable && (((c & 1u) == 0u) == positive);
    if (is_lower) sh.lower |= 1u << c;
    if (usable && !is_lower) sh.upper |= 1u << c;
}

__device__ __forceinline__ bool shaft_meets(const Shaft &sh, const NodeDev &b)
{
    const float plane[6] = {b.lox, b.hix, b.loy, b.hiy, b.loz, b.hiz};
    float s_lo = kShaftS0, s_hi = kShaftS1;
#pragma unroll
    for (uint32_t c = 0; c < 6u; ++c) {
        const float q = __builtin_fmaf(plane[c], sh.inv[c], sh.off[c]);
        s_lo = fmaxf(s_lo, (sh.lower >> c) & 1u ? q : kShaftS0);
        s_hi = fminf(s_hi, (sh.upper >> c) & 1u ? q : kShaftS1);
    }
    return !(s_lo > s_hi);   // a NaN can only accept
}

// wave-wide minimum / maximum over the lanes, as a scalar: six data-parallel-primitive steps on the vector unit (shifts
// within the rows of 16 lanes, then lane 15 of a row to the next row, lane 31 to the upper half; lanes a step does not
// reach keep their value) leave the result in lane 63.  (Through LDS — six ds_bpermute per reduction — the tile's six
// bounds were 36 LDS round trips in probe_kernel's path.)
// (inline assembly: through the builtins each step is four instructions — a copy, the shifted copy, a NaN-quieting
//  maximum, the minimum —; s_nop 1: a DPP operand written by the instruction before needs two wait states)
#define RTX_DPP_REDUCE(name, insn)                                                                                          \
    __device__ __forceinline__ float name(float v)                                                                          \
    {                                                                                                                       \
        asm volatile("s_nop 1\n\t" insn " %0, %0, %0 row_shr:1 row_mask:0xf bank_mask:0xf\n\t"                              \
                     "s_nop 1\n\t" insn " %0, %0, %0 row_shr:2 row_mask:0xf bank_mask:0xf\n\t"                              \
                     "s_nop 1\n\t" insn " %0, %0, %0 row_shr:4 row_mask:0xf bank_mask:0xf\n\t"                              \
                     "s_nop 1\n\t" insn " %0, %0, %0 row_shr:8 row_mask:0xf bank_mask:0xf\n\t"                              \
                     "s_nop 1\n\t" insn " %0, %0, %0 row_bcast:15 row_mask:0xa bank_mask:0xf\n\t"                           \
                     "s_nop 1\n\t" insn " %0, %0, %0 row_bcast:31 row_mask:0xc bank_mask:0xf\n\t"                           \
                     "s_nop 1" : "+v"(v));                                                                                  \
        return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 63));                                            \
    }
RTX_DPP_REDUCE(wave_min, "v_min_f32_dpp")
RTX_DPP_REDUCE(wave_max, "v_max_f32_dpp")
#undef RTX_DPP_REDUCE
// a value every lane holds, moved to a scalar register (the builtin is typed int: the bits go through, not the value)
__device__ __forceinline__ float uniform(float v)
{
    return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(v)));
}
__device__ __forceinline__ uint32_t wave_sum(uint32_t v)
{
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m);
    return v;
}

#if RTX_ABLATION
#include "rtx_j1_ablation.hpp"
#endif

// probe_kernel's probing walk of a one-surface tile with a cut: the tile's hit pixels towards one light point, through the
// cut's entry form in LDS; returns the records the walk fetched.  (Inlined: as a CALLED function — to keep its registers
// out of probe_kernel's, which every tile of a frame pays for — one bench run in three FAILED on the GPU box; not pursued.)
template <bool FAST, bool SPHERES>
__device__ __forceinline__ uint32_t probe_cut_walk(const NodeRec RTX_CONSTANT *nodes, const TriRec RTX_CONSTANT *tris,
                                                             const ShadeRec *shade, const uint32_t *l_entries, uint32_t n_cut,
                                                             uint32_t n_global, const float *light_point, bool hit, float hx, float hy,
                                                             float hz)
{
    const float vx = light_point[0] - hx, vy = light_point[1] - hy, vz = light_point[2] - hz;     // main.rs:201-202, as shadow_ray_at
    float dist_light, sx, sy, sz;
    (void)length_and_direction(vx, vy, vz, dist_light, sx, sy, sz);
    LaneRay sr = make_ray(hit, hx, hy, hz, sx, sy, sz);
    sr.limit = dist_light;
    WaveCounters probe;
    uint32_t first_entry = 0u;
    (void)any_hit_cut<true, FAST, SPHERES>(nodes, tris, shade, l_entries, n_cut, sr, probe, n_global, false, first_entry);
    return (uint32_t)(probe.node_visits + probe.tri_visits);
}

// Breadth-first descent of the stream with the shaft test, one frontier node per work-item; the frontier of a level lives
// in registers (lane l holds its l-th node), the next one is gathered through LDS: one stream record per work-item, its
// own box against the shaft; a leaf that meets it becomes an entry, an inner node's two children (the next record, and
// the one its `info` names) join the next frontier.  Invariant: entries written + frontier nodes <= kMaxCut, so a level
// is one pass of the wavefront; when the next level would break it, the frontier's live nodes become entries as they are
// and the descent stops.  Entries are record ranges [begin, end) of the stream.  Returns the number of entries written;
// weight = a proxy of what one chunk's walk of the cut will fetch.
__device__ __forceinline__ uint32_t shaft_cut_binary(const NodeDev *__restrict__ nodes, uint32_t root, const Shaft &sh,
                                                     CutEntry *__restrict__ out, NodeDev *__restrict__ out_stream,
                                                     uint32_t *__restrict__ l_front, CutEntry *__restrict__ l_entries,
                                                     uint32_t lane, uint32_t &weight)
{
    // the entry once more as a record of the tile's cut stream (rtx_device.h: kCutInnerFlag)
    auto stream_record = [](uint32_t at, bool leaf, NodeDev nd) {
        if (!leaf) { nd.info = kLeafFlag | kCutInnerFlag | nd.link; nd.link = at; }
        return nd;
    };
    uint32_t my = root, n_front = 1u, n_out = 0u, w = 0u;
    const float inf = __builtin_inff();
    float ulx = inf, uly = inf, ulz = inf, uhx = -inf, uhy = -inf, uhz = -inf;      // around the roots this work-item has written
    auto around = [&](const NodeDev &nd) {
        ulx = fminf(ulx, nd.lox); uly = fminf(uly, nd.loy); ulz = fminf(ulz, nd.loz);
        uhx = fmaxf(uhx, nd.hix); uhy = fmaxf(uhy, nd.hiy); uhz = fmaxf(uhz, nd.hiz);
    };
    for (;;) {
        const bool have = lane < n_front;
        NodeDev nd = {};
        if (have) nd = nodes[my];
        const bool leaf = (nd.info >> 31) != 0u;
        const bool pass = have && shaft_meets(sh, nd);
        const unsigned long long m_pass = ballot(pass), m_exp = ballot(pass && !leaf), m_leaf = m_pass & ~m_exp;
        const uint32_t n_pass = (uint32_t)__popcll(m_pass), n_exp = (uint32_t)__popcll(m_exp), n_leaf = n_pass - n_exp;
        const unsigned long long below = (1ull << lane) - 1ull;
        if (n_out + n_leaf + 2u * n_exp > kMaxCut) {      // stop here: the passing nodes of this level are the rest of the cut
            if (pass) {
                if (kCutEntriesUsed) out[n_out + (uint32_t)__popcll(m_pass & below)] = CutEntry{my, leaf ? my + 1u : nd.link, nd};
                l_entries[n_out + (uint32_t)__popcll(m_pass & below)] = CutEntry{my, leaf ? my + 1u : nd.link, nd};
                out_stream[n_out + (uint32_t)__popcll(m_pass & below)] = stream_record(my, leaf, nd);
                around(nd);
                const uint32_t size = leaf ? 1u : nd.link - my;
                w += leaf ? 1u + 3u * nd.link : 4u + 6u * (31u - (uint32_t)__clz((int)size));
            }
            n_out += n_pass;
            break;
        }
        if (pass && leaf) {
            if (kCutEntriesUsed) out[n_out + (uint32_t)__popcll(m_leaf & below)] = CutEntry{my, my + 1u, nd};
            l_entries[n_out + (uint32_t)__popcll(m_leaf & below)] = CutEntry{my, my + 1u, nd};
            out_stream[n_out + (uint32_t)__popcll(m_leaf & below)] = nd;
            around(nd);
            w += 1u + 3u * nd.link;            // its box test and its primitive records
        }
        n_out += n_leaf;
        if (n_exp == 0u) break;
        if (pass && !leaf) {                    // children of the expanding node of rank k go to slots 2k, 2k+1
            const uint32_t k = (uint32_t)__popcll(m_exp & below);
            l_front[2u * k] = my + 1u;
            l_front[2u * k + 1u] = nd.info;     // inner node: index of its second child (scene_prep.cpp)
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        n_front = 2u * n_exp;
        my = l_front[lane];
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        __builtin_amdgcn_wave_barrier();
    }
    weight = wave_sum(w);
    if (n_out >= 2u) {   // the box around all roots: the stream's last record (walk_cut_stream reads it for cuts of two or more)
        NodeDev all;
        all.lox = wave_min(ulx); all.loy = wave_min(uly); all.loz = wave_min(ulz);
        all.hix = wave_max(uhx); all.hiy = wave_max(uhy); all.hiz = wave_max(uhz);
        all.link = 0u; all.info = 0u;
        if (lane == 0) out_stream[kMaxCut] = all;
    }
    return n_out;
}

// Where probe_kernel counts its tile's cost class (W.buckets; the layout and who zeroes it: order_tiles_kernel).
constexpr uint32_t kHistShardsLog = 8u, kHistShards = 1u << kHistShardsLog;
constexpr uint32_t kOrderHist = kCostBuckets;                                  // first word of counting set 0
constexpr uint32_t kOrderCursor = kHistShards * kCostBuckets;                  // within a counting set
constexpr uint32_t kOrderSetWords = kOrderCursor + kCostBuckets;
// The workspace as the kernels that count see it: W.buckets moved to counting set `set` (0 or 1), so that
// buckets[kOrderHist + ...] is that set's first word.  The launcher hands this to probe_kernel and count_classes_kernel,
// and order_tiles_kernel finds its own and the next pass's set through the same function.
__host__ __device__ inline StreamWorkspace counting_set(StreamWorkspace W, uint32_t set)
{
    W.buckets += set * kOrderSetWords;
    return W;
}

// WHOLE: the scene does not cut per tile (S.n_nodes > S.cut_max_nodes: shade_tiles_kernel's whole-stream form follows) — an
// instantiation of its own, so that each carries one probing walk only (the kernel is short of scalar registers)
#endif  // !RTX_RECORD_FORMS: what follows is compiled for either form
#if !defined(RTX_RECORD_FORMS)
template <bool COUNT, bool FAST, bool SPHERES, bool WHOLE, uint32_t WAVES>
__global__ void __launch_bounds__(64 * WAVES, RTX_PROBE_WAVES_PER_SIMD) probe_kernel(DeviceScene S, TileSpec ts, uint32_t tiles_x, uint32_t n_tiles,
                                                   uint32_t r, StreamWorkspace W, uint8_t *__restrict__ out,
                                                   uint32_t *__restrict__ queue, unsigned long long *__restrict__ counters,
                                                   ProbeSplit split)
{
#else
#if defined(RTX_MASKED_FORMS)
template <bool COUNT, bool FAST, bool SPHERES, bool WHOLE>
__global__ void __launch_bounds__(64, RTX_PROBE_WAVES_PER_SIMD) probe_masked_kernel(DeviceScene S, TileSpec ts, uint32_t tiles_x, uint32_t n_tiles,
                                                   uint32_t r, StreamWorkspace W, uint4 *__restrict__ out_shade, uint8_t *__restrict__ out_hits,
                                                   uint32_t *__restrict__ queue, unsigned long long *__restrict__ counters,
                                                   const RtxTileState *__restrict__ tile_states, uint32_t min_frames, float max_variance)
#else
template <bool COUNT, bool FAST, bool SPHERES, bool WHOLE>
__global__ void __launch_bounds__(64, RTX_PROBE_WAVES_PER_SIMD) probe_records_kernel(DeviceScene S, TileSpec ts, uint32_t tiles_x, uint32_t n_tiles,
                                                   uint32_t r, StreamWorkspace W, uint4 *__restrict__ out_shade, uint8_t *__restrict__ out_hits,
                                                   uint32_t *__restrict__ queue, unsigned long long *__restrict__ counters)
#endif
{
    // one wavefront per tile.  (Value-dependent, as probe_kernel's parameter is: the four-beam statements of the body, which
    // this form never runs, index arrays of WAVES entries and are then not diagnosed at their definition.)
    constexpr uint32_t WAVES = COUNT ? 1u : 1u;
    const ProbeSplit split{nullptr, 0u, 0u, 0u};
    const RecordOut out{out_shade, out_hits};
#endif
    const NodeRec RTX_CONSTANT *nodes = (const NodeRec RTX_CONSTANT *)S.nodes;
    const TriRec RTX_CONSTANT *tris = (const TriRec RTX_CONSTANT *)S.tris;
    // one wavefront per tile, WAVES independent wavefronts per workgroup (no barrier; LDS only inside shaft_cut_binary
    // and the probing walk) — or, in the workgroups of the long list, the four beams of one tile, one barrier
    static_assert(WAVES == 1u || WAVES == 4u, "one tile per workgroup, or four tiles / the four beams of a long tile");
    constexpr bool kSplits = WAVES == 4u;                        // this form is handed a long list
    __shared__ uint32_t l_front_all[WAVES][128];                 // the cut's next frontier
    __shared__ CutEntry l_entries_all[WAVES][kMaxCut];           // the tile's cut in its entry form, for the probing walk
    __shared__ float l_beam_t[kSplits ? 64 : 1];                 // long mode: the four beams' answers, by lane of the tile
    __shared__ uint32_t l_beam_idx[kSplits ? 64 : 1];
    __shared__ uint32_t l_beam_ok[WAVES];
#if RTX_ABLATION
    __shared__ __align__(16) uint32_t l_j1_block[WAVES][kJ1BlockWords];   // RTX_J1=2: a block of 64 primitive records
#endif
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave_in_group = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    uint32_t *const l_front = l_front_all[wave_in_group];
    // Workgroups [0, n_long): the long list in order, costliest first — those tiles start in the kernel's first microsecond.
    // (Up to seven idle workgroups follow, so that the ordinary ones keep their XCDs.)  An entry is a tile of the FRAME; a
    // launch that renders a share of the rows finds the tile among its own or leaves (the launcher hands a list only to
    // launches whose tiles are the frame's: rtx_kernel.hip, launch_probe).
    const uint32_t n_long = kSplits ? split.n_long : 0u, long_groups = (n_long + 7u) & ~7u;
    const bool long_mode = kSplits && blockIdx.x < n_long;
    uint32_t tile_id, tile_x, tile_y;
    if (long_mode) {
        const uint32_t entry = __builtin_amdgcn_readfirstlane(split.words[blockIdx.x]);
        const uint32_t fy = entry / tiles_x;
        tile_x = entry - fy * tiles_x;
        const uint32_t row = fy * 8u;
        if (row < ts.first_row) return;
        const uint32_t band = (row - ts.first_row) / ts.tile_stride_rows, off = (row - ts.first_row) - band * ts.tile_stride_rows;
        const uint32_t ly0 = band * ts.tile_rows + off;
        if (off >= ts.tile_rows || ly0 >= ts.local_rows) return;
        tile_y = ly0 >> 3;
        tile_id = ((((tile_y >> 3) * ((tiles_x + 7u) >> 3)) + (tile_x >> 3)) << 6) + ((tile_y & 7u) << 3) + (tile_x & 7u);
        if (tile_id >= n_tiles) return;
        if (COUNT && wave_in_group != 0u) return;     // the counted form walks a tile as one wavefront (RtxStats stays what it is)
    } else if (!kSplits) {
        // workgroups b, b + 8, ... share an XCD (MI355X_MICROARCH.md, workgroup dispatch): the XCDs are dealt runs of 64
        // consecutive tile numbers — one 64 x 64 pixel block each — so that an L2 serves neighbouring tiles' walks.  (One
        // contiguous eighth of the frame per XCD was 25-35 % slower: the upper half of a frame is sky.)
        const uint32_t k = blockIdx.x >> 3;
        tile_id = ((((k >> 6) << 3) + (blockIdx.x & 7u)) << 6) + (k & 63u);
        if (tile_id >= n_tiles) return;
        tile_xy(tile_id, tiles_x, true, tile_x, tile_y);
    } else {
        if (blockIdx.x < long_groups) return;
        // the same dealing, sixteen workgroups of four consecutive tiles per run of 64
        const uint32_t g = blockIdx.x - long_groups, k = g >> 3;
        tile_id = ((((k >> 4) << 3) + (g & 7u)) << 6) + ((k & 15u) << 2) + wave_in_group;
        if (tile_id >= n_tiles) return;
        tile_xy(tile_id, tiles_x, true, tile_x, tile_y);
        // A tile of the long list has a workgroup of its own.  Only a tile inside the rectangle around the listed ones reads
        // its bit (one dependent scalar load in front of everything else: paid by every tile of a 4096 x 4096 frame it was
        // +2.5 % on the pass; of a 1920 x 1080 frame +1 us, 1.3 %: profiles/r08/h_ab_rectangle_gate_c5.log).
        if (n_long != 0u) {
            const uint32_t ly0 = tile_y * 8u, band = ly0 < ts.tile_rows ? 0u : ly0 / ts.tile_rows;
            const uint32_t fy = (ts.first_row + band * ts.tile_stride_rows + (ly0 - band * ts.tile_rows)) >> 3;
            if (tile_x >= (split.x_range & 0xFFFFu) && tile_x <= (split.x_range >> 16) && fy >= (split.y_range & 0xFFFFu) &&
                fy <= (split.y_range >> 16) && ly0 < ts.local_rows) {
                const uint32_t t = fy * tiles_x + tile_x;
                if ((split.words[n_long + (t >> 5)] >> (t & 31u)) & 1u) return;
            }
        }
    }
#if defined(RTX_MASKED_FORMS)
    // The mask.  A tile of the rectangle (the padding of the numbering's blocks has no state and no pixel: it goes on and ends
    // as a tile without a hit) reads its state by its ROW-MAJOR number — a view's launch is TileSpec{y0, ny, ny, ny}, so the
    // local tile rows are the rectangle's — as two scalars, the states being an earlier launch's words.  Stopped: a descriptor
    // that schedules nothing (no class, no hits, no redo flag, nothing counted) and the wavefront leaves — no ray, no walk,
    // no pixel, no word of acc or hits, no histogram add, no queue entry, no counter; the same in every pass of a frame.
    if (tile_x < tiles_x && tile_y * 8u < ts.local_rows) {
        const uint2 w = *reinterpret_cast<const uint2 *>(tile_states + (tile_y * tiles_x + tile_x));
        RtxTileState state;
        state.frames = __builtin_amdgcn_readfirstlane(w.x);
        state.err = __uint_as_float(__builtin_amdgcn_readfirstlane(w.y));
        if (tile_stopped(RtxAdaptRule{min_frames, max_variance}, state)) {
            if (lane == 0) W.tiles[tile_id] = TileDesc{kNone, 0u, 0u, 0u};
            return;
        }
    }
#endif
    uint32_t px, py, ly;
    const bool in_frame = tile_pixel(S, ts, tile_x, tile_y, lane, px, py, ly);
    WaveCounters wc;
    float dx, dy, dz;
    primary_ray(S, in_frame, px, py, r, dx, dy, dz);
    // long mode: every wavefront forms the tile's 64 rays, wavefront w walks the 4 x 4 pixel quadrant w — a beam half as
    // wide meets fewer boxes and leaves.  A ray's closest hit does not depend on which rays share its wavefront (the walk
    // culls by superset, each lane tests its own candidates), so the answers are the ones one wavefront would find.
    const bool beams = long_mode && !COUNT;
    const bool walks = in_frame && (!beams || (((lane >> 5) << 1) | ((lane >> 2) & 1u)) == wave_in_group);
    LaneRay pr = make_ray(walks, S.eye[0], S.eye[1], S.eye[2], dx, dy, dz);
    ProbePhaseClock phases;   // (rtx_probes.hpp: nothing in the product; long mode: wavefront 0's, the barrier included)
    phases.mark(0);
    bool ok = true;
    if (!beams || ballot(walks) != 0ull) {      // (a beam without a pixel in the frame does not walk)
#if RTX_ABLATION
        ok = (S.j1_mode == 2u || S.j1_mode == 3u)
            ? j1_closest_hit_blocks<COUNT>(S.j1_mode, S.tris, S.shade, S.n_prims, pr, wc, lane, l_j1_block[wave_in_group])
            : closest_hit<COUNT, FAST, SPHERES>((const NodeRec RTX_CONSTANT *)S.primary_nodes, tris, S.shade, S.n_nodes, pr, wc, S.n_global);   // main.rs:187
#else
        // (the primary rays' own stream of the tree, nearest-to-the-eye child first: scene_prep.h, PreparedScene::primary_nodes)
        ok = closest_hit<COUNT, FAST, SPHERES>((const NodeRec RTX_CONSTANT *)S.primary_nodes, tris, S.shade, S.n_nodes, pr, wc, S.n_global);   // main.rs:187
#endif
    }
    if (beams) {      // the four answers meet in LDS; wavefront 0 goes on with all 64 as if it had walked them
        if (walks) { l_beam_t[lane] = pr.best_t; l_beam_idx[lane] = pr.best_idx; }
        else if ((((lane >> 5) << 1) | ((lane >> 2) & 1u)) == wave_in_group) { l_beam_t[lane] = __builtin_inff(); l_beam_idx[lane] = kNone; }
        if (lane == 0) l_beam_ok[wave_in_group] = ok ? 1u : 0u;
        __syncthreads();
        if (wave_in_group != 0u) return;
        pr.best_t = l_beam_t[lane];
        pr.best_idx = l_beam_idx[lane];
        ok = (l_beam_ok[0] & l_beam_ok[1] & l_beam_ok[2] & l_beam_ok[3]) != 0u;
    }
    phases.mark(1);
    const bool hit = ok && in_frame && pr.best_idx != kNone;
    const unsigned long long hit_mask = ballot(hit);
    const uint32_t n_hit = (uint32_t)__popcll(hit_mask);
    const uint32_t slot = __popcll(hit_mask & ((1ull << lane) - 1ull));
    const uint32_t first_idx = __builtin_amdgcn_readfirstlane(hit_mask ? __shfl(pr.best_idx, __ffsll((long long)hit_mask) - 1) : 0u);
    const bool one_surface = ballot(hit && pr.best_idx != first_idx) == 0ull;
    // a tile queued for the reference re-render by an earlier primary ray stays queued (and is not queued twice)
    uint32_t was_redo = 0u, counted = 0u;
    if (r != 0u) {
        const TileDesc old = W.tiles[tile_id];
        was_redo = old.flags & 2u;
        counted = old.pad;
    }
    uint32_t flags = one_surface ? 1u : 0u;   // bit 0: the tile's shadow rays are numbered sample-major (shade_tiles_kernel)
    if (!ok || was_redo) flags |= 2u;
    if (!ok && !was_redo && lane == 0) {
        queue[kQueueHeader + atomicAdd(&queue[kQueueRedoCount], 1u)] = tile_id;
        if (COUNT && counters) {
            atomicAdd(&counters[5], 1ull);
            if (counted) atomicAdd(&counters[0], 0ull - (unsigned long long)counted);   // the re-render counts the tile's hits itself
        }
    }
    float hx = 0.0f, hy = 0.0f, hz = 0.0f;
    const bool compact = one_surface && n_hit != 0u && (!SPHERES || S.shade[first_idx].kind == 0u);
    if (compact) flags |= kTileCompactHits;
    if (hit) {
        const ShadeRec sh = S.shade[pr.best_idx];
        HitRec h;
        h.p[0] = hx = S.eye[0] + pr.best_t * dx;                                     // p_hit, bvh.rs:69
        h.p[1] = hy = S.eye[1] + pr.best_t * dy;
        h.p[2] = hz = S.eye[2] + pr.best_t * dz;
        hit_normal<SPHERES>(sh, h.p[0], h.p[1], h.p[2], h.n[0], h.n[1], h.n[2]);     // main.rs:206
        h.rgb[0] = sh.rgb[0]; h.rgb[1] = sh.rgb[1]; h.rgb[2] = sh.rgb[2];            // main.rs:191
        h.pad[0] = h.pad[1] = h.pad[2] = 0.0f;
        if (compact) {      // (compact_hit_word) one triangle: its normal and colour once, behind the 64 hit points
            float *words = reinterpret_cast<float *>(W.hits + (size_t)tile_id * 64u);
            words[3u * slot] = h.p[0]; words[3u * slot + 1u] = h.p[1]; words[3u * slot + 2u] = h.p[2];
            if (slot == 0u) {
                words[192] = h.n[0]; words[193] = h.n[1]; words[194] = h.n[2];
                words[195] = h.rgb[0]; words[196] = h.rgb[1]; words[197] = h.rgb[2];
            }
        } else {
            W.hits[(size_t)tile_id * 64u + slot] = h;
        }
    }
    if (n_hit != 0u) W.pix_slot[(size_t)tile_id * 64u + lane] = hit ? slot : kNone;   // (a tile without a hit has no job: nothing reads its slots)
    // The tile's cut (shaft_cut above) and, from it, the tile's cost estimate: chunks x (a chunk's fixed work + what a
    // walk of the cut fetches).
    unsigned long long cost = 0;
    uint32_t n_cut = 0u;
    const uint32_t n_chunks = (n_hit * S.nb_light + 63u) / 64u;
    if (n_hit != 0u && S.nb_light != 0u && !(flags & 2u)) {
        const float inf = __builtin_inff();
        const float olx = wave_min(hit ? hx : inf), ohx = wave_max(hit ? hx : -inf);
        const float oly = wave_min(hit ? hy : inf), ohy = wave_max(hit ? hy : -inf);
        const float olz = wave_min(hit ? hz : inf), ohz = wave_max(hit ? hz : -inf);
        const float *lb = S.light_boxes + 6u * r;
        Shaft sh;
        sh.lower = 0u; sh.upper = 0u;
        shaft_constraint(sh, 0u, ohx, lb[3] - ohx, S.shaft_delta);
        shaft_constraint(sh, 1u, olx, lb[0] - olx, S.shaft_delta);
        shaft_constraint(sh, 2u, ohy, lb[4] - ohy, S.shaft_delta);
        shaft_constraint(sh, 3u, oly, lb[1] - oly, S.shaft_delta);
        shaft_constraint(sh, 4u, ohz, lb[5] - ohz, S.shaft_delta);
        shaft_constraint(sh, 5u, olz, lb[2] - olz, S.shaft_delta);
        uint32_t weight = 0u;
        // the tree proper: behind the root and the global triangles' leaf when there are any (scene_prep.cpp)
        const uint32_t root = S.n_global != 0u ? 2u : 0u;
        if (!WHOLE && root < S.n_nodes) {
            NodeDev *cut_stream = reinterpret_cast<NodeDev *>(reinterpret_cast<char *>(W.cut) + cut_stream_offset(n_tiles));
            n_cut = shaft_cut_binary(reinterpret_cast<const NodeDev *>(S.nodes), root, sh, W.cut + (size_t)tile_id * kMaxCut,
                                     cut_stream + (size_t)tile_id * kCutStreamRecords, l_front, l_entries_all[wave_in_group], lane, weight);
            // A one-surface tile with a cut — the ground in and around the mesh's shadow — is probed by a REAL walk as well:
            // its hit pixels towards light sample 0, through the cut (the entry form, out of LDS: the stream just written is
            // not to be read back through the scalar cache by the kernel that wrote it).  The cut's proxy cannot tell a tile
            // in the open (its chunks pass no root) from one in the umbra (every ray walks until it is occluded): within one
            // cost class the measured times spread 50 ... 770 us (tools/tile_timeline.py), and the costliest tiles, started
            // late, are the frame's tail.  (Keeping the walk's answers as the shading pass's chunk 0, as the whole-stream form
            // does, was measured too: the shading pass's general loop pays more for the case than a walk in a hundred saves.
            // Skipping the walk in wavefronts already at work for 6 / 12 / 25 us — tiles beside the silhouette — as well: no.)
            if (n_cut != 0u && (flags & 1u)) {
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                __builtin_amdgcn_wave_barrier();
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
                const uint32_t walked_weight = RTX_PROBE_VISIT_SCALE *
                    probe_cut_walk<FAST, SPHERES>(nodes, tris, S.shade, reinterpret_cast<const uint32_t *>(l_entries_all[wave_in_group]), n_cut,
                                                  S.n_global, S.light_points + 3u * (r * S.nb_light), hit, hx, hy, hz);
                weight = weight / 2u + walked_weight;   // (half the proxy + the walk; the walk alone, and the larger of the two: no better)
            }
        } else if (WHOLE && root < S.n_nodes) {
            // A scene of many small primitives (BASELINE configs[4]): nearly every tile's shaft meets thousands of leaves, a
            // cut of sixteen subtrees prunes nothing, and what orders such a frame well is the length of a real walk — the
            // tile's hit pixels towards light sample 0, its result unused.  No cut is written: shade_tiles_kernel's
            // whole-stream form walks the stream from its first record.  (Measured on the
            // 1M-triangle soup: 61 ms with this estimate, 65-67 ms with the cut's proxy at any cut size.)
            n_cut = 0u;   // (shade_tiles_kernel's whole-stream form does not read a cut)
            const float *lp = S.light_points + 3u * (r * S.nb_light);
            const float vx = lp[0] - hx, vy = lp[1] - hy, vz = lp[2] - hz;              // main.rs:201-202, as shadow_ray_at
            float dist_light, sx, sy, sz;
            (void)length_and_direction(vx, vy, vz, dist_light, sx, sy, sz);
            LaneRay sr = make_ray(hit, hx, hy, hz, sx, sy, sz);
            sr.limit = dist_light;
            WaveCounters probe;
            const bool walked = any_hit<true, FAST, SPHERES>(nodes, tris, S.shade, S.n_nodes, sr, probe, S.n_global);
            weight = (uint32_t)(probe.node_visits + probe.tri_visits);
            // In a FULL tile numbered sample-major these 64 rays ARE the shading pass's chunk 0 — hit pixel `lane` towards
            // light sample 0, the same origin, light point and normalisation — so their answers are kept (two words where
            // a cut would lie) and shade_tiles_kernel does not walk that chunk again: one walk in a hundred.
            if (walked && n_hit == 64u && (flags & 1u)) {
                const unsigned long long occluded = ballot(sr.best_idx != kNone);
                if (lane == 0) {
                    uint32_t *kept = reinterpret_cast<uint32_t *>(W.cut + (size_t)tile_id * kMaxCut);
                    kept[0] = (uint32_t)occluded;
                    kept[1] = (uint32_t)(occluded >> 32);
                }
                flags |= kTileChunk0Kept;
            }
        }
        cost = (unsigned long long)(kChunkFixedCost + weight) * n_chunks;
        // A tile numbered pixel-major — hit pixels on several primitives: the mesh's own surface and its silhouette — takes
        // about twice as long as a one-surface tile of the same proxy (its rays start INSIDE the boxes they walk; measured per
        // cost class with tools/tile_timeline.py: x1.9 ... x2.5), and the order and the splitting should know: the costliest
        // tiles of a frame are of this kind, and one of them started late is the frame's tail.
        if (!(flags & 1u) && n_cut != 0u) cost *= 2u;
    }
    // A tile without a hit is finished here (main.rs:235: the sums stay as they are), a queued tile belongs to the
    // reference re-render: neither is scheduled for shade_tiles_kernel (cost class kNone).
    const bool sky = n_hit == 0u && !(flags & 2u);
    if (sky) {
        const size_t pix = (size_t)tile_id * 64u + lane;
        if (r + 1u == S.nb_ray) {
            float a0 = 0.0f, a1 = 0.0f, a2 = 0.0f;                                   // main.rs:182
            if (r != 0u) { a0 = W.acc[3u * pix]; a1 = W.acc[3u * pix + 1u]; a2 = W.acc[3u * pix + 2u]; }
            // (records: a pixel of a tile that is sky for this ray keeps the hits its earlier rays counted)
            if (in_frame) store_pixel(S, S.gamma_thr, out, px, ly, a0, a1, a2, r != 0u ? kept_hits(out, pix) : 0u);
        } else if (r == 0u) {
            W.acc[3u * pix] = 0.0f; W.acc[3u * pix + 1u] = 0.0f; W.acc[3u * pix + 2u] = 0.0f;
            keep_hits(out, pix, 0u);
        }
    }
    if (lane == 0) {
        const bool count_it = !(flags & 2u);
        const uint32_t key = (sky || (flags & 2u)) ? kNone : cost_class(cost);
        // the histogram order_tiles_kernel sorts by: one add, nothing returned, in the shard of the tile number's low bits.
        // (Not in the whole-stream form, which is short of scalar registers — the add took its spills from 21 to 39 —
        //  and whose launches last tens of milliseconds: count_classes_kernel counts for it, as before.)
        if (!WHOLE && key != kNone) atomicAdd(&W.buckets[kOrderHist + (tile_id & (kHistShards - 1u)) * kCostBuckets + key], 1u);
        phases.mark(2);
        // the spare word: the tile's counted hits — or, in a timing build, what its tool reads there (rtx_probes.hpp)
        W.tiles[tile_id] = TileDesc{key, n_hit, flags | (n_cut << kTileCutShift),
                                    kTilePad == TilePad::kProbeTicks ? phases.packed()
                                    : kTilePad == TilePad::kJobTicks ? 0u : counted + (count_it ? n_hit : 0u)};
        if (COUNT) {
            flush_counters<COUNT>(counters, count_it ? (unsigned long long)n_hit : 0ull, wc);
            if (counters) {   // the scheduling pass's share of the record fetches (the probing walk is not counted)
                atomicAdd(&counters[6], wc.node_visits);
                atomicAdd(&counters[7], wc.tri_visits);
            }
        }
    }
}

#if !defined(RTX_RECORD_FORMS)
}  // namespace rtx
#endif
#endif  // first inclusion, or the record forms'
