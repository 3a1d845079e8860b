// rtx_pass_order.hpp — the render pipeline's order (rtx_kernel.hip): the workspace's counting words and who zeroes them,
// the job word, who claims which job, and the kernels that count and sort — reset_kernel, count_classes_kernel,
// order_tiles_kernel.
#pragma once
#include "rtx_pass_schedule.hpp"

namespace rtx {

// Counting sort of the scheduled tiles by cost class, costliest first.  Workspace words (W.buckets):
//   [0] number of jobs in the order   [kOrderRaisedEnd] how many of them, from the front, run raised
//   [kOrderClaim + g] claims of XCD group g (further down)
//   two counting sets, kOrderSetWords each, from [kOrderHist]; a pass works on set (pass number & 1):
//     [s * kCostBuckets + k] tiles of class k, shard s of kHistShards — probe_kernel adds 1 for its tile, in the shard
//                            of the tile number's low bits (whole-stream form: count_classes_kernel, into shard 0);   [kOrderCursor + k] tiles of class k already placed
//   [kOrderList + i] the i-th job
// Who zeroes what (no kernel of a launch only zeroes; launch n works on queue n & 1 of d_redo, rtx_device.h):
//   the counting set of pass p      by order_tiles_kernel of pass p - 1, all workgroups: its last reader is the
//                                   order_tiles_kernel of pass p - 2, its first writer the probe_kernel of pass p
//   [0], [kOrderRaisedEnd], the claims, queue[kQueueNextTile]
//                                   written by workgroup 0 of order_tiles_kernel of the SAME pass: only the shading
//                                   pass behind it reads them (next tile: the first job nobody is dealt, below)
//   queue[kQueueRedoCount] of launch n + 1
//                                   by workgroup 0 of order_tiles_kernel of launch n, every pass: its last reader is the
//                                   reference_tiles_kernel of launch n - 1; launch n appends to the other queue, over
//                                   all its passes, and its reference_tiles_kernel reads that
// The first pass and the first two launches find their words zero because the caller runs zero_launch_words (reset_kernel,
// once) when it allocates or grows a buffer, and after another pipeline used them (launch_trace_shade).  A kernel boundary
// is the only synchronisation anywhere.
// The shards: probe_kernel's wavefronts finish a few hundred tiles per microsecond, four fifths of them in ONE class on
// a 4096 x 4096 frame (262,144 tiles in 0.3 ms = 700 adds per us to that class).  Tiles in flight together have
// neighbouring numbers, hence different shards: with 256 shards a word takes under 3 adds per us, where one word per
// class would be a hot address (a returning atomic per tile on such words once cost 0.38 ms).
// One workgroup per 1024 tiles: a class's position range starts where the costlier classes end (prefix over the
// histogram); inside it each workgroup reserves a block with one atomic per class it holds, and its tiles take
// consecutive slots.  Equal classes within a wavefront are counted by one lane — neighbouring tiles mostly share a
// class — so the LDS atomics stay few.  (A single workgroup walking all tiles took 48 us of a 1.9 ms frame; one global
// atomic per tile from probe_kernel — thousands on the few addresses of the common classes — added 90 us to it.)
//
// A job is a tile or a PART of one.  The pixels of a tile accumulate independently of each other (main.rs:180-240 is
// per pixel), so a tile's hit pixels can be dealt to several workgroups — hit records [p n / P, (p + 1) n / P) to
// part p — without touching any pixel's own order of additions.  That matters when a launch has few tiles per
// workgroup (one GPU's share of an 8-GPU frame): the costliest tile alone, 100 chunks walked by 8 wavefronts, then
// outlasts everything else (tools/share_timing.py: 0.48 ms of shading for an eighth of a 1.2 ms frame).  Every class
// whose tiles cost more than kSplitShare of a workgroup's fair share of the launch's estimated cost is cut into the
// power of two of parts that brings it below, at most kMaxTileParts.
// (kOrderHist, kHistShards, kOrderCursor, kOrderSetWords: in front of probe_kernel, which counts)
constexpr uint32_t kOrderList = kOrderHist + 2u * kOrderSetWords;
// Who takes which job.  The persistent workgroups b, b + 8, b + 16, ... share an XCD and with it an L2 (workgroups are
// dealt round-robin over the eight XCDs: MI355X_MICROARCH.md, workgroup dispatch); the order is dealt to these eight
// groups in runs of kClaimRun consecutive jobs — neighbouring tiles of one cost class, or the parts of one tile — so that
// what one L2 holds (node and primitive records of one region of the scene, a tile's hit records and cut) is what its
// own compute units ask for next.  Group g's k-th claim is job ((k / run) * 8 + g) * run + k % run of the order: every
// group still goes through the order costliest first, and a group whose share is used up draws from the next group's
// ([kOrderClaim + g]: claims of group g, zeroed by order_tiles_kernel).  Speed only: any workgroup may run any job.
#ifndef RTX_CLAIM_RUN_LOG
#define RTX_CLAIM_RUN_LOG 10      // runs of 16 / 64 / 256 / 1024 / 4096 jobs: the 1M-triangle soup -1.7 / -2.3 / -3.5 / -4.3 / -3.7 %
#endif
constexpr uint32_t kOrderClaim = 8u, kClaimRunLog = RTX_CLAIM_RUN_LOG;
// Which jobs' ray loops issue ahead of the others' on their SIMD (shade_tiles_kernel: s_setprio).  A persistent launch's
// wavefronts are all of one age, so at one priority a wavefront of the pass's longest job and one of a 28 us job tie for
// the issue port; the pass is as long as its costliest jobs, and what the cheap ones give up they get back a little later.
// By cost class: the jobs of the classes that cost at least kRaisedShare of order_tiles_kernel's limit (a workgroup's
// fair share of the launch) run their ray loops at kJobLevelRaised.  The order is costliest first, so these are the jobs
// in front of one position of it ([kOrderRaisedEnd]); the claimer compares its position.
// (kRaisedShare 1/4: big_bunny 1080p -2.1 % on each of two boxes, the 1M-triangle soup -1.7 %, 4096x4096 equal, one share
//  of an 8-way frame -1.5 % and equal; 1/2 and 1: inside the parent's range; 1/8: 1080p -3.2 %, 4096x4096 +0.16 % with
//  its range above the parent's; "every workgroup's first job" instead: -1.0 %; profiles/r06/b_ab_*.log, c_ab_*.log)
// Round 6, the share by launch size: a launch with fewer than kRaisedSmallJobs jobs per workgroup (a 1080p frame has
// about 16, one share of an 8-way frame 2, a 4096 x 4096 frame 128) raises from an EIGHTH of the limit — the workgroups
// of a small launch idle at its end, which is what raising wins back, and a large one has no idle share and only pays
// for the disturbance (1/8 everywhere had put C4 above the parent's range): C3 0.762 ... 0.770 against 0.771 ... 0.786
// with a quarter everywhere, one share of 8 0.1926 ... 0.1931 against 0.1934 ... 0.1942, C4 equal, the small bunny's
// 1080p frame about +0.3 % (0.2686 ... 0.2695 against 0.2679 ... 0.2681 in the shipped build's rounds; against the
// parent it is -4.7 %)  (profiles/r07/b_ab_piece4.log, d_ab_shipped.log)
constexpr float kRaisedShare = 0.25f, kRaisedShareSmall = 0.125f, kRaisedSmallJobs = 64.0f;
constexpr uint32_t kOrderRaisedEnd = 1u;      // (words 2 .. 7 of W.buckets are spare)
constexpr uint32_t kJobLevelRaised = 2u;
__device__ __forceinline__ uint32_t claimed_index(uint32_t group, uint32_t k)
{
    return ((((k >> kClaimRunLog) << 3) + group) << kClaimRunLog) + (k & ((1u << kClaimRunLog) - 1u));
}
// the work-item that claims the jobs: the next job of its XCD's group, or of the groups after it; kNone when all are used up
// (pos: where the job's position in the order goes.  Every caller passes one; the test for null stays all the same: without
//  it the whole-stream form of shade_tiles_kernel comes out with two pairs of vector moves the other way round)
__device__ __forceinline__ uint32_t claim_job(uint32_t *__restrict__ buckets, uint32_t n_jobs, uint32_t group0, uint32_t &groups_done,
                                              uint32_t *pos)
{
    while (groups_done < 8u) {
        const uint32_t g = (group0 + groups_done) & 7u;
        const uint32_t idx = claimed_index(g, atomicAdd(&buckets[kOrderClaim + g], 1u));
        if (pos) *pos = idx;
        if (idx < n_jobs) return buckets[kOrderList + idx];
        ++groups_done;
    }
    return kNone;
}
constexpr float kSplitScaleMin = 0.25f;
// (8 until the walks got the ring and the cut stream: a part is then mostly its fixed work, and four are enough — one
//  share of an 8-way 1080p frame 0.246 -> 0.231 ms, of a 4-way / 2-way one and the whole frame equal; 16: +12 %, 2: +25 %;
//  profiles/r03/xb_ab_parts_per_tile.log)
#ifndef RTX_TILE_PARTS_MAX
#define RTX_TILE_PARTS_MAX 4
#endif
constexpr uint32_t kMaxTileParts = RTX_TILE_PARTS_MAX;               // 1 = never split
static_assert(kMaxTileParts >= 1u && kMaxTileParts <= 16u && (kMaxTileParts & (kMaxTileParts - 1u)) == 0u, "parts: a power of two <= 16");
constexpr uint32_t kNotMine = 0xFFFFFFFEu;                          // shade_tiles_kernel: a pixel of another part of the tile
// job = tile | part << 25 | log2(parts) << 28 | compact hit records << 30  (bit 31 stays clear: no job equals kNone)
constexpr uint32_t kJobTileBits = 25u, kJobTileMask = (1u << kJobTileBits) - 1u, kJobPartsShift = 28u, kJobCompactShift = 30u;
static_assert(kMaxTileParts <= 8u, "a job word holds three bits of part number and two of log2(parts)");
// lower end of cost class k (cost_class above): k = 2 floor(log2 c) + (second bit of c) + 1
__device__ __forceinline__ float class_cost(uint32_t k)
{
    if (k == 0u) return 0.0f;
    const uint32_t lz = (k - 1u) >> 1, half = (k - 1u) & 1u;
    return lz ? (float)(2u + half) * (float)(1u << (lz - 1u)) : 1.0f;
}

// The counting words of a workspace and a queue, zeroed: queue[first, end) and buckets[0, n).  Not part of a launch: the
// launches keep these words zero for each other (the table in front of kOrderList); zero_launch_words runs this once
// when a buffer is new or grown or was used by something else.
__global__ void __launch_bounds__(256) reset_kernel(uint32_t *__restrict__ queue, uint32_t first, uint32_t end,
                                                    uint32_t *__restrict__ buckets, uint32_t n)
{
    for (uint32_t i = first + threadIdx.x; i < end; i += 256u) queue[i] = 0u;
    for (uint32_t i = threadIdx.x; i < n; i += 256u) buckets[i] = 0u;
}

// The whole-stream form's histogram (its probe_kernel does not count): one workgroup per 1024 tiles, equal classes
// within a wavefront counted by one lane, one global add per class and workgroup, into shard 0 of the pass's set.
__global__ void __launch_bounds__(1024) count_classes_kernel(uint32_t n_tiles, StreamWorkspace W)
{
    __shared__ uint32_t count[kCostBuckets];
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    if (tid < kCostBuckets) count[tid] = 0u;
    __syncthreads();
    const uint32_t i = blockIdx.x * 1024u + tid;
    const uint32_t key = i < n_tiles ? W.tiles[i].first : kNone;
    unsigned long long todo = ballot(key != kNone);
    while (todo != 0ull) {
        const uint32_t k0 = __builtin_amdgcn_readfirstlane(__shfl(key, __ffsll((long long)todo) - 1));
        const unsigned long long same = ballot(key == k0);
        if (lane == (uint32_t)(__ffsll((long long)same) - 1)) atomicAdd(&count[k0], (uint32_t)__popcll(same));
        todo &= ~same;
    }
    __syncthreads();
    if (tid < kCostBuckets && count[tid] != 0u) atomicAdd(&W.buckets[kOrderHist + tid], count[tid]);
}

// hist_set: the pass's counting set; queue: the launch's queue; next_redo_count: the count word of the next launch's;
// first_claim: the first job of the order that no workgroup is dealt (shade_tiles_kernel)
__global__ void __launch_bounds__(1024) order_tiles_kernel(uint32_t n_tiles, StreamWorkspace W, uint32_t shade_grid, float split_share,
                                                           uint32_t hist_set, uint32_t first_claim, uint32_t *__restrict__ queue,
                                                           uint32_t *__restrict__ next_redo_count)
{
    __shared__ uint32_t count[kCostBuckets], start[kCostBuckets], parts_log[kCostBuckets], jobs[kCostBuckets], hist[kCostBuckets];
    __shared__ float raised_cost;             // classes that cost at least this much run their ray loops at a raised priority
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    uint32_t *const set = counting_set(W, hist_set).buckets + kOrderHist;
    uint32_t *const next_set = counting_set(W, hist_set ^ 1u).buckets + kOrderHist;
    if (tid < kCostBuckets) {
        count[tid] = 0u;
        hist[tid] = 0u;
    }
    // the histogram: every workgroup adds up the shards for itself, sixteen work-items per class
    static_assert(kHistShards % 16u == 0u && kCostBuckets == 64u, "1024 work-items: 16 shards x 64 classes at a time");
    uint32_t in_shards = 0u;
    for (uint32_t s = tid >> 6; s < kHistShards; s += 16u) in_shards += set[s * kCostBuckets + lane];
    __syncthreads();
    if (in_shards != 0u) atomicAdd(&hist[lane], in_shards);
    // what the next pass and the next launch count in, and what this pass's shade_tiles_kernel claims from
    // (the table in front of kOrderList)
    for (uint32_t w = blockIdx.x * 1024u + tid; w < kOrderSetWords; w += gridDim.x * 1024u) next_set[w] = 0u;
    if (blockIdx.x == 0) {
        if (tid < 8u) W.buckets[kOrderClaim + tid] = 0u;
        if (tid == 8u) queue[kQueueNextTile] = first_claim;
        if (tid == 9u) *next_redo_count = 0u;
    }
    const uint32_t i = blockIdx.x * 1024u + tid;
    const uint32_t key = i < n_tiles ? W.tiles[i].first : kNone;
    uint32_t slot = 0u;                       // this tile's position among the workgroup's tiles of its class
    unsigned long long todo = ballot(key != kNone);
    while (todo != 0ull) {
        const uint32_t k0 = __builtin_amdgcn_readfirstlane(__shfl(key, __ffsll((long long)todo) - 1));
        const unsigned long long same = ballot(key == k0);
        uint32_t off = 0u;
        if (lane == (uint32_t)(__ffsll((long long)same) - 1)) off = atomicAdd(&count[k0], (uint32_t)__popcll(same));
        off = __shfl(off, __ffsll((long long)same) - 1);
        if (key == k0) slot = off + (uint32_t)__popcll(same & ((1ull << lane) - 1ull));
        todo &= ~same;
    }
    __syncthreads();
    if (tid < kCostBuckets) {
        // parts per tile of this class: the same numbers in every workgroup (histogram and arguments only)
        float total = 0.0f;
        uint32_t scheduled = 0u;
        for (uint32_t k = 0; k < kCostBuckets; ++k) { total += (float)hist[k] * class_cost(k); scheduled += hist[k]; }
        // With few tiles per workgroup the makespan is quantised by whole jobs (2 or 3 of them): finer parts then pay
        // for their fixed cost, which they do not when every workgroup has many jobs to even things out
        // (tools/share_timing.py: a quarter of the share costs a full C3 frame 3 %, and gains an eighth of it 10 %).
        const float per_wg = (float)scheduled / (float)shade_grid;
        const float scale = per_wg >= 16.0f ? 1.0f : (per_wg <= 16.0f * kSplitScaleMin ? kSplitScaleMin : per_wg * (1.0f / 16.0f));
        const float limit = split_share * scale * total / (float)shade_grid;
        // ... and a part is a workgroup's fixed work plus a few chunks per wavefront: round 2 found eight parts worth it
        // only where a workgroup has fewer than three jobs, four otherwise (profiles/r02/j_ab_parts_per_tile.log); since
        // round 3's walks four is the most anywhere (kMaxTileParts)
        const uint32_t most_parts = per_wg < 3.0f ? kMaxTileParts : (kMaxTileParts < 4u ? kMaxTileParts : 4u);
        uint32_t lg = 0u;
        while ((1u << lg) < most_parts && class_cost(tid) > limit * (float)(1u << lg)) ++lg;
        parts_log[tid] = lg;
        jobs[tid] = hist[tid] << lg;
        if (tid == 0) raised_cost = limit * (per_wg < kRaisedSmallJobs ? kRaisedShareSmall : kRaisedShare);
    }
    __syncthreads();
    if (tid < kCostBuckets) {
        uint32_t before = 0u;                 // jobs of costlier classes
        for (uint32_t k = tid + 1u; k < kCostBuckets; ++k) before += jobs[k];
        const uint32_t mine = count[tid];
        start[tid] = before + ((mine ? atomicAdd(&set[kOrderCursor + tid], mine) : 0u) << parts_log[tid]);
        if (blockIdx.x == 0 && tid == 0) W.buckets[0] = before + jobs[0];
        // the order is costliest first: the raised classes' jobs are its first [kOrderRaisedEnd]
        // (written by the cheapest raised class; class_cost rises with the class, so when the costliest class does not
        //  cost that much none does, and that class writes zero: the word is written by every pass)
        const bool raised = tid != 0u && class_cost(tid) >= raised_cost;
        const bool cheaper_raised = tid > 1u && class_cost(tid - 1u) >= raised_cost;
        if (blockIdx.x == 0 && raised && !cheaper_raised) W.buckets[kOrderRaisedEnd] = before + jobs[tid];
        if (blockIdx.x == 0 && tid == kCostBuckets - 1u && !raised) W.buckets[kOrderRaisedEnd] = 0u;
    }
    __syncthreads();
    if (key != kNone) {
        const uint32_t lg = parts_log[key];
        uint32_t *dst = W.buckets + kOrderList + start[key] + (slot << lg);
        const uint32_t form = (W.tiles[i].flags & kTileCompactHits) ? 1u << kJobCompactShift : 0u;
        for (uint32_t p = 0; p < (1u << lg); ++p) dst[p] = i | (p << kJobTileBits) | (lg << kJobPartsShift) | form;
    }
}

}  // namespace rtx
