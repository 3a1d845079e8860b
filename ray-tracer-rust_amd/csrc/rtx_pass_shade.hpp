// rtx_pass_shade.hpp — the render pipeline's shading pass (rtx_kernel.hip): shade_tiles_kernel, persistent workgroups
// that pull the order's jobs costliest first, and the LDS image of such a workgroup.
//
// rtx_kernel.hip includes this file a second time, inside namespace rtxo with RTX_RECORD_FORMS defined: then the kernel's text
// alone is compiled once more, as rtxo::shade_records_kernel — the same body with `out` a RecordOut (rtx_pass_helpers.hpp).
// What differs is the job's last stretch: the store, and between a pixel's rays its hit count.  (Text compiled twice and not
// a __device__ template: called through one, the byte forms came out with other instructions than the parent commit's —
// tools/same_isa.py — and a refactoring's gate here is identical device code.)
#if !defined(RTX_PASS_SHADE_HPP) || defined(RTX_RECORD_FORMS)
#if !defined(RTX_RECORD_FORMS)
#define RTX_PASS_SHADE_HPP
#include <type_traits>
#include "rtx_probes.hpp"
#include "rtx_pass_order.hpp"

namespace rtx {

// LDS image of a workgroup (floats): light records of the current batch [4*batch], hit records
// [64][8] = {p_hit.xyz, normal.xyz, -, -}, sample results [64][res_stride], {hit count, redo flag}.
// control words of a workgroup: [0] chunks drawn, [1] redo flag, [2] grey tile, [3] job, [4 .. 11] unused (they were the
// wavefronts' run counters of a tour form that left the sources; the words behind them keep their places),
// [kCtlJobLevel] the job's level
constexpr uint32_t kCtlWords = 20u;
__host__ __device__ inline uint32_t lds_res_stride(uint32_t batch) { return batch | 1u; }   // odd: conflict-free column reads
__host__ __device__ inline uint32_t lds_floats(uint32_t batch)
{
    return kLightStride * batch + 64u * kHitStride + 64u * lds_res_stride(batch) + 64u * 4u + kCtlWords + kCutWords * kMaxCut + 256u;
}

// Without the primary phase the kernel fits the 64 VGPRs of 8 wavefronts per SIMD (4 workgroups per CU): 53 VGPRs, no
// scratch in the shipped build; when it first went in, 8 per SIMD measured 2.22 ms against 2.28 ms at 6 (C3).
#ifndef RTX_SHADE_WAVES_PER_SIMD
#define RTX_SHADE_WAVES_PER_SIMD 8
#endif

// WHOLE: the scene is too large for per-tile cuts (probe_kernel: kCutMaxNodes) and every chunk walks the whole stream —
// a kernel of its own, so that neither form carries the other's registers: the whole-stream loop is three scalar
// instructions per record shorter than the loop over a cut's ranges (9 % of a frame of the 1M-triangle soup), and the
// cut form has a path for chunks with nothing to walk.
// Wavefronts per SIMD the register allocation must allow: the whole-stream form lives on resident wavefronts (its walks
// are long chains of dependent scalar loads: 8, i.e. 64 vector and 78 scalar registers; at 6 the 1M-triangle soup takes
// 20 % longer); the cut form, whose frames are mostly chunks that walk little or nothing, does better with the registers
// of 6 (fewer scalar registers spilled to lanes: -3 % on big_bunny 4096x4096, -7 % on the ground-only frame, 1080p equal).
// (A full tile's registers — hit record, the origin's part of the ground's certificate — are the open-ground loop's
//  alone.  With the general chunk loop working on them too, the 64 vector registers of 8 wavefronts per SIMD keep nine of
//  them alive across the walk and ten in scratch instead of one: big_bunny 4096x4096 -1.2 %, the ground-only frame
//  -1.7 %, one share of an 8-way 1080p frame -2.6 %, the 1080p frame +0.5 % for the form kept (four interleaved rounds,
//  profiles/r02/j_ab_full_tile_registers.log).)
// (The cut form at 6 was 3-7 % faster than at 8 while a cheap job was bound by its serial stretches; since the open
//  ground's chunks are bound by their vector instructions — the loop of their own below — 8 is, although ten vector
//  registers then live in scratch: big_bunny 4096x4096 -4.6 %, the ground-only frame -2 %, one share of an 8-way 1080p
//  frame -2.5 %, the 1080p frame +0.8 % (six interleaved rounds); 4: +17 ... +29 %.
//  profiles/r02/j_ab_waves_per_simd_again.log)
#ifndef RTX_SHADE_CUT_WAVES_PER_SIMD
#define RTX_SHADE_CUT_WAVES_PER_SIMD 8
#endif
// s_setprio levels of a job: its serial stretches (its loads into LDS, the ordered sums, the store) run at kShadePriority,
// its ray loops at the job's own level — 0, or kJobLevelRaised for the launch's costly jobs, whose
// ray loops then issue ahead of the other jobs' serial stretches as well (the serial stretches at 3 instead, above the
// raised loops: +0.4 % on the "first job" rule, not taken; profiles/r06/b_ab_*.log)
constexpr int kShadePriority = 1;
constexpr uint32_t kCtlJobLevel = 12u;        // l_ctl word: the job's level, published with the job id
// s_setprio takes an immediate: a uniform branch over the levels
__device__ __forceinline__ void set_wave_priority(uint32_t level)
{
    switch (level) {
    case 0u: __builtin_amdgcn_s_setprio(0); break;
    case 1u: __builtin_amdgcn_s_setprio(1); break;
    case 2u: __builtin_amdgcn_s_setprio(2); break;
    default: __builtin_amdgcn_s_setprio(3); break;
    }
}
#endif  // !RTX_RECORD_FORMS: what follows is compiled for either form
template <bool COUNT, bool FAST, int NW, bool SPHERES, bool WHOLE>
__global__ void __launch_bounds__(64 * NW, COUNT ? 1 : (WHOLE ? RTX_SHADE_WAVES_PER_SIMD : RTX_SHADE_CUT_WAVES_PER_SIMD))
#if !defined(RTX_RECORD_FORMS)
shade_tiles_kernel(DeviceScene S, TileSpec ts, uint32_t batch, uint32_t tiles_x, uint32_t n_tiles, uint32_t r,
                   StreamWorkspace W, uint8_t *__restrict__ out, uint32_t *__restrict__ queue,
                   unsigned long long *__restrict__ counters)
{
#else
shade_records_kernel(DeviceScene S, TileSpec ts, uint32_t batch, uint32_t tiles_x, uint32_t n_tiles, uint32_t r,
                     StreamWorkspace W, uint4 *__restrict__ out_shade, uint8_t *__restrict__ out_hits, uint32_t *__restrict__ queue,
                     unsigned long long *__restrict__ counters)
{
    const RecordOut out{out_shade, out_hits};
#endif
    extern __shared__ __align__(16) float lds[];
    constexpr bool kRecords = std::is_same<decltype(out), const RecordOut>::value;
    // whether the lane's pixel has a hit record in this job (l_pix's fourth word: a slot, kNone or kNotMine)
    auto pix_hit = [](const float *l_pix, uint32_t lane) { return reinterpret_cast<const uint32_t *>(l_pix)[4u * lane + 3u] < 64u; };
    float *const l_light = lds;
    float *const l_hit = l_light + kLightStride * batch;
    float *const l_res = l_hit + 64u * kHitStride;
    const uint32_t res_stride = lds_res_stride(batch);
    float *const l_pix = l_res + 64u * res_stride;                                    // per pixel: running sums r,g,b + hit slot
    uint32_t *const l_ctl = reinterpret_cast<uint32_t *>(l_pix + 64u * 4u);           // [1] redo flag, [3] tile
    uint32_t *const l_cut = l_ctl + kCtlWords;                                                // the tile's cut: CutEntry records
    float *const l_thr = reinterpret_cast<float *>(l_cut + kCutWords * kMaxCut);        // the 256 gamma thresholds (eight dependent
    for (uint32_t k = threadIdx.x; k < 256u; k += 64u * NW) l_thr[k] = S.gamma_thr[k];   // reads per channel per pixel: LDS, not L1)
#if RTX_ABLATION
    uint32_t *const l_j1_win = reinterpret_cast<uint32_t *>(l_thr + 256u);             // RTX_J1=1 only (launch_probe sizes LDS for it)
    if (S.j1_mode == 1u && threadIdx.x < 2u) l_j1_win[threadIdx.x] = 0u;               // "no window" until a job stages one
#endif

    const NodeRec RTX_CONSTANT *nodes = (const NodeRec RTX_CONSTANT *)S.nodes;
    const TriRec RTX_CONSTANT *tris = (const TriRec RTX_CONSTANT *)S.tris;
    // the first global triangle's plane, fetched once (rtx_traverse.hpp: plane_rules_out)
    const TriRec RTX_CONSTANT *planes = (const TriRec RTX_CONSTANT *)S.planes;
    const bool have_plane = planes != nullptr;
    TriRec plane0 = {};
    if (have_plane) {
        plane0.v0[0] = planes->v0[0]; plane0.v0[1] = planes->v0[1]; plane0.v0[2] = planes->v0[2];
        plane0.e1[0] = planes->e1[0]; plane0.e1[1] = planes->e1[1]; plane0.e1[2] = planes->e1[2];
        plane0.e2[0] = planes->e2[0]; plane0.e2[1] = planes->e2[1]; plane0.e2[2] = planes->e2[2];
        plane0.bmin[0] = planes->bmin[0];
    }
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    WaveCounters wc;
    const float denom = (float)(S.nb_ray * S.nb_light);                              // main.rs:211
    const DenomDiv denom_d = denom_div(denom);
    static_assert(sizeof(HitRec) == kHitStride * sizeof(float), "the LDS hit record is the HBM hit record");

    JobTimeline timeline;     // (rtx_probes.hpp; this and the jobs' phase clocks are nothing in the product)
    // The next job is claimed by the work-item that claims them while the current job's last batch runs (its position in
    // the list is requested when the batch's rays start, turned into a job id when its ordered sums start), so that the
    // claim's latency — an atomic's round trip, then a load that depends on it — does not stand between two jobs, and no
    // earlier than that so that the list stays a dynamic one.  (Claiming two jobs ahead at the top of a job tied the costliest jobs, which come first, to workgroups three
    // at a time: +17 % on a 1080p frame.)
    const uint32_t n_jobs = W.buckets[0];
    uint32_t job_ahead = kNone, q_ahead = 0u;
    static_assert(kCtlJobLevel >= 4u && kCtlJobLevel < kCtlWords, "the level's word is one of the control words");
    const uint32_t raised_end = W.buckets[kOrderRaisedEnd];   // the jobs in front of this position run their ray loops raised
    uint32_t pos_ahead = 0u;     // job_ahead's position in the order
    bool have_ahead = false;
    // (the whole-stream form only — scenes whose records do not fit an XCD's L2; measured on one box, interleaved, runs of 16:
    //  the 1M-triangle soup -1.7 %, and with the cut form big_bunny 4096x4096 -0.4 %, 1080p +2 %, the ground-only frame +10 %)
    constexpr bool xcd_queues = WHOLE;
    const uint32_t group0 = blockIdx.x & 7u;
    uint32_t groups_done = 0u, g_ahead = 0u;      // (state of the work-item that claims the jobs)
    // A workgroup's FIRST job is dealt, not claimed: workgroup b takes job b of the order, and the claims start behind
    // the grid (order_tiles_kernel sets the cursor there).  The grid's workgroups start within a microsecond of each
    // other, and a thousand claims on one word take about ten (88 adds per us): the order's first jobs, the costliest,
    // started that late.  Measured: the shading pass 9 ... 10 us shorter on a 1080p frame of either bunny and on the
    // 4096 x 4096 frame (profiles/r07/a_ab_pieces.log).
    if (!xcd_queues) {
        job_ahead = blockIdx.x < n_jobs ? W.buckets[kOrderList + blockIdx.x] : kNone;
        pos_ahead = blockIdx.x;
        have_ahead = true;
    }
    // the light points are the same for every job of a launch (main.rs:194-196: sample i of primary ray r): when one batch
    // holds them all they are staged once, not once per job (a global round trip of 2.4 us in front of every job's rays)
    const bool lights_once = S.nb_light <= batch;
    if (lights_once)
        for (uint32_t k = threadIdx.x; k < kLightStride * S.nb_light; k += 64u * NW) l_light[k] = S.light_tour[kLightStride * (r * S.nb_light) + k];
    for (;;) {
        if (threadIdx.x == 0) {
            if (!have_ahead) {   // the first job, and after jobs without a last phase
                if (xcd_queues) {
                    job_ahead = claim_job(W.buckets, n_jobs, group0, groups_done, &pos_ahead);
                } else {
                    const uint32_t q = atomicAdd(&queue[kQueueNextTile], 1u);        // q-th job, costliest class first
                    job_ahead = q < n_jobs ? W.buckets[kOrderList + q] : kNone;
                    pos_ahead = q;
                }
            }
            l_ctl[3] = job_ahead;
            l_ctl[kCtlJobLevel] = pos_ahead < raised_end ? kJobLevelRaised : 0u;
            have_ahead = false;
            l_ctl[1] = 0u;
            timeline.next(job_ahead, kJobTileMask, W.tiles);
        }
        __syncthreads();
        const uint32_t job = __builtin_amdgcn_readfirstlane(l_ctl[3]);
        if (job == kNone) break;
        // A job's short serial stretches (its loads into LDS, the ordered sums, the store) are what the other wavefronts
        // of its workgroup wait for at barriers: they issue ahead of the other workgroups' ray loops on the same SIMD
        __builtin_amdgcn_s_setprio(kShadePriority);
        JobPhaseClock phases;
        phases.mark(0);
        // part `part` of 2^parts_log of the tile: its hit records [h0, h0 + n_hit), the pixels they belong to, and (part 0)
        // the tile's pixels without a hit
        const uint32_t tile_id = job & kJobTileMask, part = (job >> kJobTileBits) & 7u, parts_log = (job >> kJobPartsShift) & 3u;
        const bool compact = ((job >> kJobCompactShift) & 1u) != 0u;
        uint32_t tile_x, tile_y;
        tile_xy(tile_id, tiles_x, true, tile_x, tile_y);
        // A whole tile's job requests everything it needs from HBM at once — the tile's descriptor, all 64 of its hit-record
        // slots, its pixel slots, its cut list — and sorts it out when it is there: waiting for the descriptor first, to ask
        // only for the records that exist, made two dependent round trips in front of every such job.  A PART of a tile
        // (costly tiles only) keeps the two steps: sixteen parts would each fetch the whole tile's records.
        const float *tile_hits = reinterpret_cast<const float *>(W.hits + (size_t)tile_id * 64u);
        float hit_words[(64u * kHitStride + 64u * NW - 1u) / (64u * NW)];
        if (parts_log == 0u) {
#pragma unroll
            for (uint32_t j = 0; j < sizeof(hit_words) / sizeof(float); ++j) {
                const uint32_t k = threadIdx.x + j * 64u * NW;
                const uint32_t at = compact ? compact_hit_word(k / kHitStride, k % kHitStride) : k;
                hit_words[j] = (k < 64u * kHitStride && at != kNone) ? tile_hits[at] : 0.0f;
            }
        }
        static_assert(kCutWords * kMaxCut <= 64u * NW, "one word of the cut per work-item");
        // (the cut's entries go to LDS only where something reads them there — kCutEntriesUsed; the whole-stream form keeps
        //  two words of answers in their place)
        const uint32_t cut_word = threadIdx.x < (WHOLE ? 2u : (kCutEntriesUsed ? kCutWords * kMaxCut : 0u))
                                      ? reinterpret_cast<const uint32_t *>(W.cut + (size_t)tile_id * kMaxCut)[threadIdx.x] : 0u;
        const uint32_t pix_word = wave == 0u ? W.pix_slot[(size_t)tile_id * 64u + lane] : kNone;   // (with the rest: not behind the descriptor)
        const TileDesc td = W.tiles[tile_id];
        const uint32_t n_all = __builtin_amdgcn_readfirstlane(td.n_hit);
        const uint32_t h0 = (part * n_all) >> parts_log;
        const uint32_t n_hit = (((part + 1u) * n_all) >> parts_log) - h0;
        const uint32_t tflags = __builtin_amdgcn_readfirstlane(td.flags);
        const bool sample_major = (tflags & 1u) != 0u;
        const bool skip = (tflags & 2u) != 0u;      // already queued for the reference re-render
        const uint32_t n_cut = (tflags >> kTileCutShift) & 0xFFu;
        // the tile's cut as a stream (rtx_device.h: kCutInnerFlag), behind the tiles' entry arrays
        const NodeRec RTX_CONSTANT *cut_stream = (const NodeRec RTX_CONSTANT *)(
            reinterpret_cast<const char *>(W.cut) + cut_stream_offset(n_tiles)) + (size_t)tile_id * kCutStreamRecords;
        // whole-stream form: chunk 0 of a full sample-major tile was walked by probe_kernel (its probing walk); the answers
        // lie where a cut would (words 0 and 1: work-items 0 and 1 of wavefront 0, which is the wavefront that has chunk 0)
        const bool chunk0_kept = WHOLE && (tflags & kTileChunk0Kept) != 0u && parts_log == 0u &&
                                 n_hit == 64u && sample_major;
        const uint32_t kept_lo = __builtin_amdgcn_readlane(cut_word, 0), kept_hi = __builtin_amdgcn_readlane(cut_word, 1);
        if (!skip) {
            if (parts_log == 0u) {
#pragma unroll
                for (uint32_t j = 0; j < sizeof(hit_words) / sizeof(float); ++j) {
                    const uint32_t k = threadIdx.x + j * 64u * NW;
                    if (k < n_hit * kHitStride) l_hit[k] = hit_words[j];
                }
            } else {                                                                 // the part's records [h0, h0 + n_hit) -> LDS [0, n_hit)
                for (uint32_t k = threadIdx.x; k < n_hit * kHitStride; k += 64u * NW) {
                    const uint32_t at = compact ? compact_hit_word(h0 + k / kHitStride, k % kHitStride) : h0 * kHitStride + k;
                    l_hit[k] = at != kNone ? tile_hits[at] : 0.0f;
                }
            }
            if (kCutEntriesUsed && threadIdx.x < kCutWords * n_cut) l_cut[threadIdx.x] = cut_word;
#if RTX_ABLATION
            if (!WHOLE && S.j1_mode == 1u) {      // the stream window of this tile's cut -> LDS (rtx_j1_ablation.hpp)
                __syncthreads();
                j1_stage_window(S.nodes, l_cut, n_cut, l_j1_win, 64u * NW);
            }
#endif
            if (wave == 0) {
                const size_t pix = (size_t)tile_id * 64u + lane;
                float a0 = 0.0f, a1 = 0.0f, a2 = 0.0f;                               // main.rs:182
                if (r != 0u) { a0 = W.acc[3u * pix]; a1 = W.acc[3u * pix + 1u]; a2 = W.acc[3u * pix + 2u]; }
                l_pix[4u * lane] = a0; l_pix[4u * lane + 1u] = a1; l_pix[4u * lane + 2u] = a2;
                // the pixel's hit record within this part; kNone: no hit and the pixel is this part's; kNotMine: another part's
                const uint32_t g = pix_word;
                reinterpret_cast<uint32_t *>(l_pix)[4u * lane + 3u] =
                    g == kNone ? (part == 0u ? kNone : kNotMine) : (g - h0 < n_hit ? g - h0 : kNotMine);
            }
            __syncthreads();
            phases.mark(1);
            if (wave == 0) {   // grey tile (every BASELINE scene): the three channel sums are the same f32 sequence
                const uint32_t slot = reinterpret_cast<const uint32_t *>(l_pix)[4u * lane + 3u];
                const bool hit = slot < 64u;
                const float *h = l_hit + kHitStride * (hit ? slot : 0u);
                const float cr = h[6], cg = h[7], cb = h[8];
                const float a0 = l_pix[4u * lane], a1 = l_pix[4u * lane + 1u], a2 = l_pix[4u * lane + 2u];
                const bool grey_tile = ballot(hit && !(cr == cg && cg == cb && cr >= 0.0f && a0 == a1 && a1 == a2)) == 0ull;
                if (lane == 0) l_ctl[2] = grey_tile ? 1u : 0u;   // read behind the barrier that publishes the light points
            }
            // a full tile numbered sample-major: the open-ground loop below keeps each lane's hit record in registers; cut
            // form only: the whole-stream form has no registers to spare
            const bool full_tile = !WHOLE && sample_major && n_hit == 64u;
            float my_hit[7] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
            PlaneOrigin my_plane = {0.0f, 0.0f};          // the origin's part of the ground's certificate (plane_rules_out)
            if (n_hit != 0u) {                                                        // else main.rs:235
                for (uint32_t b0 = 0; b0 < S.nb_light; b0 += batch) {                 // main.rs:193, in batches that fit LDS
                    const uint32_t bc = (S.nb_light - b0 < batch) ? S.nb_light - b0 : batch;
                    if (!lights_once) {
                        for (uint32_t k = threadIdx.x; k < kLightStride * bc; k += 64u * NW)
                            l_light[k] = S.light_tour[kLightStride * (r * S.nb_light + b0) + k]; // main.rs:194-196 (hoisted to the host)
                    }
                    if ((WHOLE || RTX_CUT_DRAW_MIN != 0) && threadIdx.x == 0) l_ctl[0] = 0u;   // chunks drawn so far (behind the first NW)
                    // (not read: without this dead line the per-job prologue's scalar instructions come out in another
                    //  order — the kernel is that sensitive, and a refactoring's gate is identical device code)
                    [[maybe_unused]] const uint32_t n_chunks = (n_hit * bc + 63u) >> 6;
                    __syncthreads();   // (also publishes the grey flag)
                    // A tile with an empty cut is through its rays in 10 us: the next job's position in the list is requested
                    // now, by the work-item that claims the jobs, and turned into a job id when the ordered sums start —
                    // neither round trip is waited for.  (A costly job claims when its sums start: claimed a hundred
                    // microseconds ahead, the costliest jobs are tied to workgroups two at a time, +13 % on a 1080p frame.)
                    const bool claim_early = n_cut == 0u;
                    if (threadIdx.x == 0 && b0 + batch >= S.nb_light && claim_early) {
                        if (!xcd_queues) {
                            q_ahead = atomicAdd(&queue[kQueueNextTile], 1u);
                        } else if (groups_done < 8u) {
                            g_ahead = (group0 + groups_done) & 7u;
                            q_ahead = atomicAdd(&W.buckets[kOrderClaim + g_ahead], 1u);
                        }
                    }
                    phases.mark(2);
                    // phase 2: shadow rays, one work-item per (hit pixel, sample)
                    const uint32_t total = n_hit * bc;
                    const uint32_t div = sample_major ? n_hit : bc;
                    const bool grey_tile = __builtin_amdgcn_readfirstlane(l_ctl[2]) != 0u;
                    // (read here, once per batch, not held in a scalar register across the job)
                    const uint32_t job_level = __builtin_amdgcn_readfirstlane(l_ctl[kCtlJobLevel]);
                    // (carrying the chunk's quotient and remainder in scalar registers, advanced by additions, removes
                    //  the division per ray and was measured 3 % SLOWER on C2/C4, same box, interleaved runs)
                    // Ray number / div in six full-rate instructions: trunc((ray + 0.5) * fl(1/div)) is the exact quotient
                    // for ray < 2^22 — the product's error, 2^-23 (ray + 0.5)/div, stays below the 0.5/div that separates
                    // it from the next integer (checked exhaustively for the domain, ray < 8320, div <= 128).  The
                    // general 32-bit division costs three quarter-rate multiplies and a dozen more instructions.
                    const float inv_div = 1.0f / (float)div;
                    set_wave_priority(job_level);
                    // The chunks of a full grey tile of the open ground — no subtree in its cut, the ground the only global
                    // triangle — in a loop of their own: ray, the ground's certificate, the sample's contribution; nothing
                    // of the walk is in it (no copies into the general loop's registers, none of its spilled scalars).  A
                    // chunk the short way does not settle (the normalisation's or the certificate's) is where the general
                    // loop takes over.  These tiles are bound by their vector instructions: 0.36 ms of a 0.41 ms
                    // ground-only frame, 81 % of big_bunny 4096x4096.
                    uint32_t c_first = wave * 64u;
                    uint32_t first_entry = 0u;        // the cut's entry this wavefront's next walk begins with (walk_cut)
                    if (!WHOLE && full_tile && grey_tile && n_cut == 0u && have_plane && S.n_global == 1u && denom_d.usable) {
                        // A full tile numbered sample-major: chunk c is light sample c for the 64 pixels, lane l carries pixel l
                        // in every chunk, and the ray number needs no division.  The lane's hit record (my_hit[0..2] p_hit,
                        // [3..5] normal, [6] red) and the origin's part of the ground's certificate (my_plane) stay in registers
                        // that are this loop's alone: loaded here, dead behind it.  (Reading the other tiles' records per chunk
                        // into the same registers, to spare the general loop the copies where the two ways meet: +3 %.)
#pragma unroll
                        for (uint32_t k = 0; k < 7u; ++k) my_hit[k] = l_hit[kHitStride * lane + k];
                        my_plane = plane_origin(plane0, my_hit[0], my_hit[1], my_hit[2]);
                        // The four words of the plane record this loop reads, as values of their own: the record came in with
                        // one eight-word scalar load, the register allocator treats it as one eight-register value, and when
                        // it spills that value around the walk (any change to the walk's registers decides that) this loop
                        // reloads all eight words per chunk.  (The empty statement makes the copies opaque to the compiler.)
                        float pn0 = plane0.e1[0], pn1 = plane0.e1[1], pn2 = plane0.e1[2], pkd = plane0.bmin[0];
                        float dd_ = uniform(denom_d.d), dy_ = uniform(denom_d.y);   // (formed by vector instructions: same in every lane)
                        asm volatile("" : "+s"(pn0), "+s"(pn1), "+s"(pn2), "+s"(pkd), "+s"(dd_), "+s"(dy_));
                        for (; c_first < total; c_first += 64u * NW) {
                            const float4 lp = *reinterpret_cast<const float4 *>(l_light + kLightStride * (c_first >> 6));   // chunk = walk position
                            const uint32_t sample = __float_as_uint(lp.w);
                            const float vx = lp.x - my_hit[0], vy = lp.y - my_hit[1], vz = lp.z - my_hit[2];   // p - orig
                            float dist_light, sx, sy, sz;
                            if (!length_and_direction(vx, vy, vz, dist_light, sx, sy, sz)) break;    // main.rs:201-202
                            // (the certificate's "magnitude" half: these origins lie on the ground, "moving away" certifies
                            //  none of them; a tile above the ground falls to the general loop and the whole certificate)
                            const float sd = __builtin_fmaf(sz, pn2, __builtin_fmaf(sy, pn1, sx * pn0));           // plane_rules_out's sd
                            if (ballot(!(my_plane.lhs < fabsf(sd) - pkd)) != 0ull) break;
                            const float lnd = fabsf(my_hit[3] * sx + my_hit[4] * sy + my_hit[5] * sz);            // main.rs:207
                            // main.rs:211 by div_denom's short steps (the loop is entered with a usable divisor; a chunk with
                            // a numerator outside their range is the general loop's — no loop-invariant flag is tested here:
                            // as lane masks in spilled scalar registers two of them cost four reloads per chunk)
                            const float x = my_hit[6] * lnd;
                            if (ballot(!(x == 0.0f || (x >= 0x1p-60f && x <= 0x1p60f))) != 0ull) break;
                            const float q0 = x * dy_;
                            const float q1 = __builtin_fmaf(__builtin_fmaf(-dd_, q0, x), dy_, q0);
                            l_res[__umul24(lane, res_stride) + sample] = __builtin_fmaf(__builtin_fmaf(-dd_, q1, x), dy_, q1);
                        }
                    }
                    // A wavefront DRAWS its next chunk (a counter in LDS) instead of being dealt every NW-th, in the whole-stream
                    // form and in tiles of the cut form that walk.  Walks differ in length by an order of magnitude (a chunk in
                    // the open: a dozen records; one whose rays all end in the mesh: fifty to two hundred — the split by outcome
                    // in DESIGN.md section 4), and a job ends when its slowest wavefront does: the 1M-triangle soup -7 %.
                    // (Not in the counted cut form: a wavefront's walk begins at the cut entry where its previous chunk found
                    //  its occluder — first_entry — so with drawn chunks the records a chunk walks depend on which wavefront
                    //  drew it, and box_tests / tri_tests / the visit counts of one frame differed from launch to launch by
                    //  0.1 %, the bytes never.  Dealt chunks make RtxStats reproducible; the counted form is not timed.)
                    const bool kDrawChunks = WHOLE || (!COUNT && RTX_CUT_DRAW_MIN != 0 && n_cut >= RTX_CUT_DRAW_MIN);
                    for (uint32_t c0 = c_first; c0 < total; ) {
                        const bool valid = c0 + lane < total;
                        const uint32_t quo = (uint32_t)(((float)(c0 + lane) + 0.5f) * inv_div);
                        const uint32_t rem = (c0 + lane) - __umul24(quo, div);
                        ShadowRay sr;   // (declared, then assigned: as an initialisation the walk's registers are allocated differently)
                        sr = shadow_ray_at(l_hit, l_light, valid, valid ? quo : 0u, valid ? rem : 0u, sample_major);
                        const bool no_ground = have_plane &&
                            ballot(sr.ray.active && !plane_rules_out(plane0, sr.ray.ox, sr.ray.oy, sr.ray.oz, sr.ray.dx, sr.ray.dy, sr.ray.dz)) == 0ull;
                        // A chunk with nothing to walk — no subtree in the tile's cut, and the ground (the only global triangle)
                        // ruled out from its plane — is lit; what is left of the walk's own prologue is its refusal of hard
                        // directions (closest_hit: such a tile is re-rendered against the reference's tree).  Three of four
                        // chunks of a frame of the default scene are of this kind.
                        bool ok;
                        const bool nothing_to_walk = n_cut == 0u && !WHOLE && (S.n_global == 0u || (S.n_global == 1u && no_ground));
                        if (WHOLE && chunk0_kept && c0 == 0u && b0 == 0u) {   // probe_kernel has walked these rays: its answers
                            const unsigned long long occluded = ((unsigned long long)kept_hi << 32) | kept_lo;
                            sr.ray.best_idx = ((occluded >> lane) & 1ull) ? 0u : kNone;
                            ok = true;
                        } else if (nothing_to_walk) {
                            ok = sr.not_hard || ballot(sr.ray.active && direction_is_hard(sr.ray.dx, sr.ray.dy, sr.ray.dz)) == 0ull;
                        } else {
                            ray_cull_constants(sr.ray);                              // main.rs:204
#if RTX_ABLATION
                            if (WHOLE && S.j1_mode == 1u)
                                ok = j1_any_hit_whole_vec<COUNT, SPHERES>(S.nodes, nodes, tris, S.shade, S.n_nodes, l_j1_win, sr.ray, wc, S.n_global, no_ground);
                            else
#endif
                            if (WHOLE)
                                ok = any_hit<COUNT, FAST, SPHERES, true>(nodes, tris, S.shade, S.n_nodes, sr.ray, wc, S.n_global, no_ground);
#if RTX_ABLATION
                            else if (S.j1_mode == 1u)
                                ok = j1_any_hit_cut_vec<COUNT, SPHERES>(S.nodes, nodes, tris, S.shade, l_cut, n_cut, l_j1_win, sr.ray, wc, S.n_global, no_ground);
#endif
                            else
                                ok = any_hit_cut_stream<COUNT, FAST, SPHERES, true>(nodes, tris, S.shade, cut_stream, n_cut, sr.ray, wc, S.n_global, no_ground, first_entry);
                        }
                        if (!ok && lane == 0) l_ctl[1] = 1u;
                        if (grey_tile) shadow_result_grey<!WHOLE>(l_hit, l_res, res_stride, sr, denom_d);   // (whole-stream form: no registers to spare, +0.7 %)
                        else shadow_result(l_hit, l_res, res_stride, sr);
                        if (kDrawChunks) {
                            uint32_t drawn = 0u;
                            if (lane == 0) drawn = atomicAdd(&l_ctl[0], 1u);
                            c0 = (NW + __builtin_amdgcn_readfirstlane(drawn)) * 64u;
                        } else {
                            c0 += 64u * NW;
                        }
                    }
                    __builtin_amdgcn_s_setprio(kShadePriority);
                    __syncthreads();
                    phases.mark(3);
                    // phase 3: ordered accumulation, one work-item per pixel (wave 0)
                    if (wave == 0) {
                        if (threadIdx.x == 0 && b0 + batch >= S.nb_light) {          // last batch: the claimed position -> job id
                            if (!xcd_queues) {
                                if (!claim_early) q_ahead = atomicAdd(&queue[kQueueNextTile], 1u);
                                job_ahead = q_ahead < n_jobs ? W.buckets[kOrderList + q_ahead] : kNone;
                                pos_ahead = q_ahead;
                            } else if (groups_done >= 8u) {
                                job_ahead = kNone;
                            } else {
                                if (!claim_early) {
                                    g_ahead = (group0 + groups_done) & 7u;
                                    q_ahead = atomicAdd(&W.buckets[kOrderClaim + g_ahead], 1u);
                                }
                                const uint32_t idx = claimed_index(g_ahead, q_ahead);
                                if (idx < n_jobs) {
                                    job_ahead = W.buckets[kOrderList + idx];
                                    pos_ahead = idx;
                                } else {       // the group's share is used up: on to the next group's (the end of a launch only)
                                    ++groups_done;
                                    job_ahead = claim_job(W.buckets, n_jobs, group0, groups_done, &pos_ahead);
                                }
                            }
                            have_ahead = true;
                        }
                        const uint32_t slot = reinterpret_cast<const uint32_t *>(l_pix)[4u * lane + 3u];
                        const bool hit = slot < 64u;
                        float acc_r = l_pix[4u * lane], acc_g = l_pix[4u * lane + 1u], acc_b = l_pix[4u * lane + 2u];
                        const float *h = l_hit + kHitStride * (hit ? slot : 0u);
                        const float cr = h[6], cg = h[7], cb = h[8];
                        if (hit) {
                            const float *res = l_res + slot * res_stride;
                            if (grey_tile) {
                                // i ascending, main.rs:209-216: res[i] = (color.red * lnd) / denom, +0.0 when occluded.  Eight
                                // reads in flight per step: this chain of additions is what one wavefront does alone
                                // while seven wait
                                uint32_t i = 0;
                                for (; i + 8u <= bc; i += 8u) {
                                    const float q0 = res[i], q1 = res[i + 1u], q2 = res[i + 2u], q3 = res[i + 3u];
                                    const float q4 = res[i + 4u], q5 = res[i + 5u], q6 = res[i + 6u], q7 = res[i + 7u];
                                    acc_r = acc_r + q0; acc_r = acc_r + q1; acc_r = acc_r + q2; acc_r = acc_r + q3;
                                    acc_r = acc_r + q4; acc_r = acc_r + q5; acc_r = acc_r + q6; acc_r = acc_r + q7;
                                }
                                for (; i < bc; ++i) acc_r = acc_r + res[i];
                                acc_g = acc_r;
                                acc_b = acc_r;
                            } else {
                                for (uint32_t i = 0; i < bc; ++i) {                   // i ascending, main.rs:209-216
                                    const float lnd = res[i];
                                    if (!(lnd < 0.0f)) {
                                        acc_r = acc_r + ((cr * lnd) / denom);
                                        acc_g = acc_g + ((cg * lnd) / denom);
                                        acc_b = acc_b + ((cb * lnd) / denom);
                                    }
                                }
                            }
                            l_pix[4u * lane] = acc_r; l_pix[4u * lane + 1u] = acc_g; l_pix[4u * lane + 2u] = acc_b;
                        }
                    }
                    __syncthreads();   // results and light points are overwritten by the next batch
                    phases.mark(4);
                }
            }
            if (wave == 0) {
                const bool mine = reinterpret_cast<const uint32_t *>(l_pix)[4u * lane + 3u] != kNotMine;
                if (l_ctl[1] != 0u) {   // a hard shadow direction: reference_tiles_kernel redoes the tile and counts its hits
                    // (whatever the tile's other parts store is overwritten by it; the first part to get here queues the tile)
                    if (lane == 0 && !(atomicOr(&W.tiles[tile_id].flags, 2u) & 2u)) {
                        queue[kQueueHeader + atomicAdd(&queue[kQueueRedoCount], 1u)] = tile_id;
                        if (COUNT && counters) {
                            atomicAdd(&counters[5], 1ull);
                            atomicAdd(&counters[0], 0ull - (unsigned long long)td.pad);
                        }
                    }
                } else if (r + 1u < S.nb_ray) {
                    const size_t pix = (size_t)tile_id * 64u + lane;
                    if (mine) {
                        W.acc[3u * pix] = l_pix[4u * lane]; W.acc[3u * pix + 1u] = l_pix[4u * lane + 1u];
                        W.acc[3u * pix + 2u] = l_pix[4u * lane + 2u];
                        if (kRecords) keep_hits(out, pix, (r != 0u ? kept_hits(out, pix) : 0u) + (pix_hit(l_pix, lane) ? 1u : 0u));
                    }
                } else {
                    uint32_t px, py, ly;
                    if (tile_pixel(S, ts, tile_x, tile_y, lane, px, py, ly) && mine) {
                        const float cr = l_pix[4u * lane], cg = l_pix[4u * lane + 1u], cb = l_pix[4u * lane + 2u];
                        // (records: this ray's hit is the pixel's slot; the earlier rays' hits are where the sums were)
                        uint32_t n_hits = 0u;
                        if (kRecords) n_hits = (r != 0u ? kept_hits(out, (size_t)tile_id * 64u + lane) : 0u) + (pix_hit(l_pix, lane) ? 1u : 0u);
                        if (ballot(!(cr == cg && cg == cb)) == 0ull) {   // grey sums: one search of the thresholds, not three
                            store_grey(S, out, px, ly, cr, cg, cb, quantise(l_thr, cr), n_hits);
                        } else {
                            store_pixel(S, l_thr, out, px, ly, cr, cg, cb, n_hits);
                        }
                    }
                }
            }
        }
        __syncthreads();   // the control words and hit records are rewritten by the next tile
        phases.mark(5);
        if (threadIdx.x == 0 && n_cut == 0u && n_hit != 0u && !skip) phases.add_to(W.tiles);   // the jobs of tiles with an empty cut
    }
    if (COUNT && lane == 0) flush_counters<COUNT>(counters, 0ull, wc);
}

#if !defined(RTX_RECORD_FORMS)
}  // namespace rtx
#endif
#endif  // first inclusion, or the record forms'
