// rtx_pass_helpers.hpp — the render pipeline's tile and pixel helpers (rtx_kernel.hip): the tile numbering, a pixel's
// primary ray, a job's shadow rays and their results, the launch's divisor, the gamma search and the pixel store, the
// counters' flush.  Used by every pass and by the ablation library's kernel forms.
#pragma once
#include "rtx_traverse.hpp"

namespace rtx {

namespace {

// LDS hit record of the fused kernel: p_hit xyz, normal xyz, colour rgb, 3 spare floats
constexpr uint32_t kHitStride = 12u;
// Hit records of a tile whose hit pixels all lie on ONE triangle (the ground, walls: nine tiles in ten of the default
// scene) in a compact form: the 64 slots hold 64 x 12 bytes of hit POINTS, then once the normal and the colour they share —
// 792 bytes instead of 3072, written by probe_kernel and read by the tile's job (a 4096 x 4096 frame: 0.38 GB each way).
// The job word says which form it is (the descriptor arrives with the records, not before them).  compact_hit_word: where
// word k of the full form (record k / 12, word k % 12) lies in the compact one; kNone: a padding word (zero).
__device__ __forceinline__ uint32_t compact_hit_word(uint32_t record, uint32_t word)
{
    return word < 3u ? record * 3u + word : (word < 9u ? 192u + word - 3u : kNone);
}

// byte of a linear channel: number of thresholds (b >= 1) that are <= x  (color.rs:28-33).  -inf counts as +inf: it is
// the one negative whose power is a number — powf(-inf, 1 / 2.2) = +inf, byte 255; every other negative gives NaN, byte 0
__device__ __forceinline__ uint32_t quantise(const float *__restrict__ thr, float x)
{
    if (x == -__builtin_inff()) x = __builtin_inff();
    uint32_t b = 0;
#pragma unroll
    for (uint32_t step = 128; step; step >>= 1)
        if (x >= thr[b + step]) b += step;
    return b;
}

// pixel of lane `lane` in tile (tile_x, tile_y) of this launch; false when it lies outside the frame share
__device__ __forceinline__ bool tile_pixel(const DeviceScene &S, const TileSpec &ts, uint32_t tile_x, uint32_t tile_y,
                                           uint32_t lane, uint32_t &px, uint32_t &py, uint32_t &ly)
{
    px = tile_x * 8u + (lane & 7u);
    ly = tile_y * 8u + (lane >> 3);
    const uint32_t band = ly / ts.tile_rows;
    py = ts.first_row + band * ts.tile_stride_rows + (ly - band * ts.tile_rows);
    return px < S.width && ly < ts.local_rows && py < S.height;
}

// Tile numbering of the two-pass pipeline: 8 x 8 tiles (64 x 64 pixels) form a block whose tiles are numbered
// consecutively, blocks row by row — consecutive tile numbers (what one XCD is dealt: probe_kernel's workgroups, the
// runs of shade_tiles_kernel's order) are then a compact patch of the frame, not a strip eight pixels high, and their
// rays meet the same part of the scene.  The blocks of the right and lower edge are padded: a tile outside the frame
// has no pixel (tile_pixel) and ends as a tile without a hit.  (tile_xy with blocks = false: row-major, the single-kernel
// ablation variants.)
__host__ __device__ inline uint32_t numbered_tiles(uint32_t tiles_x, uint32_t tiles_y)
{
    return ((tiles_x + 7u) / 8u) * ((tiles_y + 7u) / 8u) * 64u;
}
__device__ __forceinline__ void tile_xy(uint32_t tile_id, uint32_t tiles_x, bool blocks, uint32_t &tx, uint32_t &ty)
{
    if (blocks) {
        const uint32_t blocks_x = (tiles_x + 7u) >> 3, b = tile_id >> 6, j = tile_id & 63u;
        const uint32_t by = b / blocks_x, bx = b - by * blocks_x;
        tx = bx * 8u + (j & 7u);
        ty = by * 8u + (j >> 3);
    } else {
        ty = tile_id / tiles_x;
        tx = tile_id - ty * tiles_x;
    }
}

// create_rays (main.rs:151-178) + Ray::new (ray.rs:12-17) for ray r of pixel (px, py)
__device__ __forceinline__ void primary_ray(const DeviceScene &S, bool in_frame, uint32_t px, uint32_t py, uint32_t r,
                                            float &dx, float &dy, float &dz)
{
    float s0 = 0.0f, s1 = 0.0f;
    if (in_frame) {
        const uint32_t k = (px * S.width + py + r) % S.n_samples;                    // :162,165 (u32)
        const float2 s = S.samples[k];
        s0 = s.x;
        s1 = s.y;
    }
    const float a = (float)px - (float)S.width / 2.0f + s0;                          // :161-162
    const float b = (float)py - (float)S.height / 2.0f + s1;                         // :164-165
    const float rx = (a * S.cu[0] + b * S.cv[0]) - S.distance * S.cw[0];             // :160-167
    const float ry = (a * S.cu[1] + b * S.cv[1]) - S.distance * S.cw[1];
    const float rz = (a * S.cu[2] + b * S.cv[2]) - S.distance * S.cw[2];
    float rn;
    (void)length_and_direction(rx, ry, rz, rn, dx, dy, dz);                          // ray.rs:15: sqrt, three divisions (bit for bit)
}

// One shadow ray of phase 2: ray number -> (compacted hit pixel, walk position of the batch), origin = the pixel's hit
// point, direction = towards the light point at that position (main.rs:194-202).  l_light holds the batch's records of
// DeviceScene::light_tour, four words per position: the point, and the index within the batch of the sample it is — the
// column of l_res its result belongs to, which arrives with the point's own read.
constexpr uint32_t kLightStride = 4u;
struct ShadowRay {
    LaneRay ray;
    uint32_t hp, si;     // si: the SAMPLE (the result's column), not the position
    bool valid;          // the lane carries a ray (ray.active is consumed by the any-hit walk)
    bool not_hard;       // wave-uniform: no lane's direction is "hard" (length_and_direction took its short way)
};

// (quo, rem) = ray number / and % the tile's divisor, see the callers; indices are small: 24-bit multiplies are full rate
__device__ __forceinline__ ShadowRay shadow_ray_at(const float *__restrict__ l_hit, const float *__restrict__ l_light,
                                                   bool valid, uint32_t quo, uint32_t rem, bool sample_major)
{
    ShadowRay s;
    s.hp = sample_major ? rem : quo;     // compacted hit pixel
    const uint32_t pos = sample_major ? quo : rem;     // walk position within the batch
    const float *h = l_hit + __umul24(kHitStride, s.hp);
    const float4 lp = *reinterpret_cast<const float4 *>(l_light + __umul24(kLightStride, pos));
    s.si = __float_as_uint(lp.w);
    const float hx = h[0], hy = h[1], hz = h[2];
    const float vx = lp.x - hx, vy = lp.y - hy, vz = lp.z - hz;                      // p - orig
    float dist_light, sx, sy, sz;
    s.not_hard = length_and_direction(vx, vy, vz, dist_light, sx, sy, sz);            // main.rs:202; Ray::new, main.rs:201 -> ray.rs:15
    s.ray = make_ray_bare(valid, hx, hy, hz, sx, sy, sz);     // the caller adds the culling constants when the ray walks
    s.ray.limit = dist_light;
    s.valid = valid;
    return s;
}

// |n.l| when the sample is lit, the marker when it is occluded (main.rs:206-232)
__device__ __forceinline__ void shadow_result(const float *__restrict__ l_hit, float *__restrict__ l_res,
                                              uint32_t res_stride, const ShadowRay &s)
{
    const float *h = l_hit + kHitStride * s.hp;
    const LaneRay &r = s.ray;
    const float lnd = fabsf(h[3] * r.dx + h[4] * r.dy + h[5] * r.dz);               // main.rs:207
    const bool lit = r.best_idx == kNone;       // main.rs:219-231 through any_hit: an index is kept only for an occluder
    if (s.valid) l_res[__umul24(s.hp, res_stride) + s.si] = lit ? lnd : kOccluded;
}

// x / denom for the divisor a whole launch shares (denom = NB_RAY * NB_LIGHT_SAMPLE, main.rs:211): the compiler's IEEE
// division without its range scaling and fix-up — y = 1/denom once per kernel (reciprocal_ieee's steps), then q0 = x*y,
// r0 = x - denom*q0, q1 = q0 + r0*y, r1 = x - denom*q1, q = q1 + r1*y with fused residuals, five instructions instead of
// eleven.  The left-out steps do nothing for x = 0 and for 2^-60 <= x <= 2^60 with 1 <= denom <= 2^30 (rtx_traverse.hpp:
// divide3_ieee): the same instructions on the same values, the same bits — tools/div_denom_check.hip compares every
// binary32 x in [2^-60, 2^60] for eighteen divisors.  A wavefront with a lane outside (tiny, huge, infinite — a caller's
// colour may be anything —, negative, NaN) divides.
struct DenomDiv { float d, y; bool usable; };
__device__ __forceinline__ DenomDiv denom_div(float denom)
{
    DenomDiv dd;
    dd.d = denom;
    const float y0 = __builtin_amdgcn_rcpf(denom);
    dd.y = __builtin_fmaf(y0, __builtin_fmaf(-denom, y0, 1.0f), y0);
    dd.usable = denom >= 1.0f && denom <= 0x1p30f;
    return dd;
}
__device__ __forceinline__ float div_denom(float x, const DenomDiv &dd)
{
    if (!dd.usable || ballot(!(x == 0.0f || (x >= 0x1p-60f && x <= 0x1p60f))) != 0ull) return x / dd.d;
    const float q0 = x * dd.y;
    const float r0 = __builtin_fmaf(-dd.d, q0, x);
    const float q1 = __builtin_fmaf(r0, dd.y, q0);
    const float r1 = __builtin_fmaf(-dd.d, q1, x);
    return __builtin_fmaf(r1, dd.y, q1);
}

// The same for a tile whose hit pixels are all grey (red == green == blue >= 0, equal running sums): the lane stores
// the sample's contribution (color.red * lnd) / denom itself (main.rs:211-215), so that the ordered accumulation,
// which one wavefront does alone, is left with the additions.  Contributions are >= 0 (or NaN), the marker is not.
template <bool FAST_DIV>
__device__ __forceinline__ void shadow_result_grey(const float *__restrict__ l_hit, float *__restrict__ l_res,
                                                   uint32_t res_stride, const ShadowRay &s, const DenomDiv &dd)
{
    const float *h = l_hit + __umul24(kHitStride, s.hp);
    const LaneRay &r = s.ray;
    const float lnd = fabsf(h[3] * r.dx + h[4] * r.dy + h[5] * r.dz);               // main.rs:207
    const bool lit = r.best_idx == kNone;
    // an occluded sample contributes (black * 1.0) / denom = +0.0 (main.rs:226): adding it changes no sum of this kind
    // (they start at +0.0 and only grow), so the ordered accumulation needs no test
    const float c = FAST_DIV ? div_denom(h[6] * lnd, dd) : (h[6] * lnd) / dd.d;
    if (s.valid) l_res[__umul24(s.hp, res_stride) + s.si] = lit ? c : 0.0f;
}

__device__ __forceinline__ void store_pixel(const DeviceScene &S, const float *__restrict__ thr, uint8_t *__restrict__ out,
                                            uint32_t px, uint32_t ly, float r, float g, float b)
{
    uint8_t *p = out + ((size_t)ly * S.width + px) * 3u;                             // put_pixel, main.rs:293-294
    p[0] = (uint8_t)quantise(thr, r);
    p[1] = (uint8_t)quantise(thr, g);
    p[2] = (uint8_t)quantise(thr, b);
}
__device__ __forceinline__ void store_pixel(const DeviceScene &S, uint8_t *__restrict__ out, uint32_t px, uint32_t ly,
                                            float r, float g, float b)
{
    store_pixel(S, S.gamma_thr, out, px, ly, r, g, b);
}

// Where a launch's pixels go, as the type of the kernels' bodies' `out`: uint8_t * — RGB8, three byte stores per pixel —
// or RecordOut: one 16-byte RtxPixelShade record per pixel (the three ordered sums, their three bytes, the hit count; record
// ly * width + px), and, for a scene with more than one ray per pixel, the per-pixel hit counts the passes of a launch
// hand on as they hand on the sums in StreamWorkspace::acc (tiles x 64 bytes, indexed as acc's pixels; saturating at 255).
// store_pixel with a hit count is the one store both have: the bytes ignore the count.
struct RecordOut {
    uint4 *shade;
    uint8_t *hits;       // read and written only when nb_ray > 1
};
__device__ __forceinline__ uint32_t kept_hits(const uint8_t *, size_t) { return 0u; }
__device__ __forceinline__ uint32_t kept_hits(const RecordOut &out, size_t pix) { return out.hits[pix]; }
__device__ __forceinline__ void keep_hits(const uint8_t *, size_t, uint32_t) {}
__device__ __forceinline__ void keep_hits(const RecordOut &out, size_t pix, uint32_t n) { out.hits[pix] = (uint8_t)(n < 255u ? n : 255u); }
__device__ __forceinline__ void store_pixel(const DeviceScene &S, const float *__restrict__ thr, uint8_t *__restrict__ out,
                                            uint32_t px, uint32_t ly, float r, float g, float b, uint32_t)
{
    store_pixel(S, thr, out, px, ly, r, g, b);
}
__device__ __forceinline__ void store_record(const DeviceScene &S, const RecordOut &out, uint32_t px, uint32_t ly, float r,
                                             float g, float b, uint32_t qr, uint32_t qg, uint32_t qb, uint32_t n_hit)
{
    out.shade[(size_t)ly * S.width + px] = make_uint4(__float_as_uint(r), __float_as_uint(g), __float_as_uint(b),
                                                      qr | (qg << 8) | (qb << 16) | ((n_hit < 255u ? n_hit : 255u) << 24));
}
__device__ __forceinline__ void store_pixel(const DeviceScene &S, const float *__restrict__ thr, const RecordOut &out,
                                            uint32_t px, uint32_t ly, float r, float g, float b, uint32_t n_hit)
{
    store_record(S, out, px, ly, r, g, b, quantise(thr, r), quantise(thr, g), quantise(thr, b), n_hit);
}
// the grey-tile shortcut's store: one search has given all three bytes
__device__ __forceinline__ void store_grey(const DeviceScene &S, uint8_t *__restrict__ out, uint32_t px, uint32_t ly, float,
                                           float, float, uint32_t q, uint32_t)
{
    uint8_t *p = out + ((size_t)ly * S.width + px) * 3u;             // put_pixel, main.rs:293-294
    p[0] = (uint8_t)q; p[1] = (uint8_t)q; p[2] = (uint8_t)q;
}
__device__ __forceinline__ void store_grey(const DeviceScene &S, const RecordOut &out, uint32_t px, uint32_t ly, float r,
                                           float g, float b, uint32_t q, uint32_t n_hit)
{
    store_record(S, out, px, ly, r, g, b, q, q, q, n_hit);
}

template <bool COUNT>
__device__ __forceinline__ void flush_counters(unsigned long long *__restrict__ counters, unsigned long long primary_hits,
                                               const WaveCounters &wc)
{
    if (!counters) return;
    if (primary_hits) atomicAdd(&counters[0], primary_hits);
    atomicAdd(&counters[1], wc.box_tests);
    atomicAdd(&counters[2], wc.tri_tests);
    atomicAdd(&counters[3], wc.node_visits);
    atomicAdd(&counters[4], wc.tri_visits);
}

}  // namespace

}  // namespace rtx
