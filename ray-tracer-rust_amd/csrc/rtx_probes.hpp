// rtx_probes.hpp — the timing instrumentation of the render kernels (rtx_kernel.hip), out of their bodies.
//
// Three compile-time switches, each for one tool of tools/; same pixels, but they cost time, so they are named in
// rtx_build_switches_text like every other switch and are 0 in the product:
//   RTX_EXPERIMENT_TIMELINE      tools/tile_timeline.py   every job adds its duration to its tile's descriptor
//   RTX_EXPERIMENT_PHASES        tools/job_phases.py      where a job of a tile with an empty cut spends its time
//   RTX_EXPERIMENT_PROBE_PHASES  tools/probe_phases.py    a tile's primary walk and the rest of probe_kernel's work on it
// All of them report through the spare word of the tiles' descriptors, TileDesc::pad (rtx_debug_tile_descs): kTilePad says
// what the word holds in this build.  The kernels hold one plain call per site; with its switch at 0 a type below is
// empty and its calls are nothing.
#pragma once
#include "rtx_traverse.hpp"

#ifndef RTX_EXPERIMENT_TIMELINE
#define RTX_EXPERIMENT_TIMELINE 0
#endif
#ifndef RTX_EXPERIMENT_PHASES
#define RTX_EXPERIMENT_PHASES 0
#endif
#ifndef RTX_EXPERIMENT_PROBE_PHASES
#define RTX_EXPERIMENT_PROBE_PHASES 0
#endif

namespace rtx {

// What probe_kernel leaves in TileDesc::pad:
//   kHitCount    the product: the primary hits counted for the tile so far (taken back when the tile is re-rendered)
//   kJobTicks    zero — the tile's jobs add their durations (JobTimeline), the first six tiles' words take JobPhaseClock's sums
//   kProbeTicks  ProbePhaseClock::packed()
enum class TilePad { kHitCount, kJobTicks, kProbeTicks };
constexpr TilePad kTilePad = RTX_EXPERIMENT_PROBE_PHASES                        ? TilePad::kProbeTicks
                             : (RTX_EXPERIMENT_TIMELINE || RTX_EXPERIMENT_PHASES) ? TilePad::kJobTicks
                                                                                  : TilePad::kHitCount;

// shade_tiles_kernel, state of the work-item that claims the jobs: a job's duration (100 MHz ticks, claim to next claim) is
// added to its tile's spare word.
struct JobTimeline {
#if RTX_EXPERIMENT_TIMELINE
    uint32_t tile = kNone;
    unsigned long long t0 = 0;
    // job: the job word just published, or kNone at the end; tile_mask: the tile number's bits of a job word
    __device__ __forceinline__ void next(uint32_t job, uint32_t tile_mask, TileDesc *tiles)
    {
        const unsigned long long now = wall_clock64();
        if (tile != kNone) atomicAdd(&tiles[tile].pad, (uint32_t)(now - t0));
        tile = job == kNone ? kNone : (job & tile_mask);
        t0 = now;
    }
#else
    __device__ __forceinline__ void next(uint32_t, uint32_t, TileDesc *) {}
#endif
};

// shade_tiles_kernel, every work-item: the six points of a job (its start; hit records, pixel slots and cut in LDS; light
// points in LDS and the next claim requested; the rays done; the ordered sums done; the store done — the last batch's, when
// there are several), 100 MHz ticks.  add_to: the five stretches are added to the spare words of the first five tiles'
// descriptors and one job is counted in the sixth's.
struct JobPhaseClock {
#if RTX_EXPERIMENT_PHASES
    unsigned long long t[6] = {0, 0, 0, 0, 0, 0};
    __device__ __forceinline__ void mark(int k) { t[k] = wall_clock64(); }
    __device__ __forceinline__ void add_to(TileDesc *tiles) const
    {
        for (int k = 0; k < 5; ++k) atomicAdd(&tiles[k].pad, (uint32_t)(t[k + 1] - t[k]));
        atomicAdd(&tiles[5].pad, 1u);
    }
#else
    __device__ __forceinline__ void mark(int) {}
    __device__ __forceinline__ void add_to(TileDesc *) const {}
#endif
};

// probe_kernel: a tile's primary walk (marks 0 .. 1) and everything behind it — the cut's descent, the probing walk, the
// histogram — (marks 1 .. 2) in 10 ns ticks, as the low and the high half of one word, each saturating at 0xFFFF.
struct ProbePhaseClock {
#if RTX_EXPERIMENT_PROBE_PHASES
    unsigned long long t[3] = {0, 0, 0};
    __device__ __forceinline__ void mark(int k) { t[k] = wall_clock64(); }
    __device__ __forceinline__ uint32_t packed() const
    {
        const uint32_t walk = (uint32_t)(t[1] - t[0]), rest = (uint32_t)(t[2] - t[1]);
        return (walk > 0xFFFFu ? 0xFFFFu : walk) | ((rest > 0xFFFFu ? 0xFFFFu : rest) << 16);
    }
#else
    __device__ __forceinline__ void mark(int) {}
    __device__ __forceinline__ uint32_t packed() const { return 0u; }
#endif
};

}  // namespace rtx
