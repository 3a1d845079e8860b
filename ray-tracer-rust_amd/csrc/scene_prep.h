// scene_prep.h — host-side preparation of a scene for the gfx950 tracer kernel.
//
// Pure C++ (no HIP): everything here runs on the CPU once per scene and is
// testable without a device.  It is the host half of the product path, not a
// fallback: nothing in this file traces a ray.
//
// Record layouts are shared with the kernel (rtx_kernel.hip includes this file).
#pragma once

#include <cmath>
#include <cstdint>
#include <vector>

#include "../../include/rtx.h"

// one statement for the host's compiler and the device's, where both must give the same bits
#if defined(__HIP__)
#define RTX_HOST_DEVICE __host__ __device__
#else
#define RTX_HOST_DEVICE
#endif

namespace rtx {

// Triangle::get_sample — triangle.rs:113-127.  The third weight is v*sqrt(u), as in the reference (the weights do not sum
// to one); kept on purpose.  Compiled by the host (light_sample, scene_prep.cpp) and by the device (rtxl::
// light_points_kernel, rtx_light.hip) from this one text: with -ffp-contract=off on both sides and the device's correctly
// rounded square root every operation rounds once, in this order, and the two agree bit for bit.
RTX_HOST_DEVICE inline void light_sample_point(const float v0[3], const float v1[3], const float v2[3], float u, float v,
                                               float out[3])
{
    const float su = sqrtf(u);
    const float sv = sqrtf(v);
    const float w0 = 1.0f - su;
    const float w1 = su * (1.0f - sv);
    const float w2 = v * su;
    for (int k = 0; k < 3; ++k)
        out[k] = w0 * v0[k] + w1 * v1[k] + w2 * v2[k];
}
// Distance of two light points for the tour of a call's light (light_tour_order_f32 on the host, rtxt::tour_kernel on the
// device): f32, the squares added in this order, one correctly rounded square root.  One text for both compilers, as
// light_sample_point is; D(a, b) and D(b, a) are the same bits (the differences are each other's negations).
RTX_HOST_DEVICE inline float tour_distance(const float a[3], const float b[3])
{
    const float e0 = a[0] - b[0];
    const float e1 = a[1] - b[1];
    const float e2 = a[2] - b[2];
    return sqrtf((e0 * e0 + e1 * e1) + e2 * e2);
}
// Draw i of a seeded sample table (rtx_scene_reseed; the kernel: rtx_samples.hip): splitmix64 in closed form.  The state of
// draw i is seed + (i + 1) * 0x9E3779B97F4A7C15 mod 2^64 — what rtxh_gen_samples' running sum holds at its draw i — mixed by
// the same two xor-shift-multiplies and the final shift; the value is the top 24 bits times 2^-24, a conversion and a
// product that are both exact.  Pair k of a table is (draw 2k, draw 2k + 1).  Integer arithmetic and two exact f32 steps:
// one text for both compilers, as light_sample_point is, and nothing for either to round differently.
RTX_HOST_DEVICE inline float sample_statement(uint64_t seed, uint64_t i)
{
    uint64_t z = seed + (i + 1ull) * 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z ^= z >> 31;
    return static_cast<float>(static_cast<uint32_t>(z >> 40)) * 0x1p-24f;
}
// The mean of N frames (rtx_render_view_mean, rtx_accum_*_device; the kernels: rtx_accum.hip).  Three statements, each one
// text for both compilers, as sample_statement is: rtxh_accum_add / rtxh_accum_resolve on the host, rtxc::accum_add_kernel /
// rtxc::accum_resolve_kernel on the device.
// quantise_statement: the byte of a linear channel, the number of thresholds thr[1 .. 255] that are <= x by the eight
// dependent reads of the render and view kernels' search (rtx_pass_helpers.hpp: quantise; color.rs:28-33).  -inf counts as
// +inf (powf(-inf, 1 / 2.2) = +inf: byte 255); a NaN and every other negative value lose every comparison: byte 0.
RTX_HOST_DEVICE inline uint32_t quantise_statement(const float *thr, float x)
{
    if (x == -__builtin_inff()) x = __builtin_inff();
    uint32_t b = 0;
    for (uint32_t step = 128; step; step >>= 1)
        if (x >= thr[b + step]) b += step;
    return b;
}
// accum_add_statement: frame k's record into the pixel's accumulator.  first: the three words of `linear` copied bit for
// bit (a NaN keeps its payload) and hit_frames = (hits != 0); what *acc held is not read and may be anything.  Otherwise
// sum[c] = sum[c] + linear[c], one f32 addition per channel, and hit_frames += (hits != 0), a plain u32 addition.
RTX_HOST_DEVICE inline void accum_add_statement(bool first, const RtxPixelShade &shade, RtxAccumPixel *acc)
{
    const uint32_t hit = shade.hits != 0 ? 1u : 0u;
    if (first) {
        __builtin_memcpy(acc->sum, shade.linear, 12);
        acc->hit_frames = hit;
        return;
    }
    for (int c = 0; c < 3; ++c) acc->sum[c] = acc->sum[c] + shade.linear[c];
    acc->hit_frames = acc->hit_frames + hit;
}
// accum_resolve_statement: linear[c] = sum[c] / (float)n_frames, one correctly rounded f32 division (never a product with
// a reciprocal: sum / 3 and sum * (1 / 3) differ in the last bit for a third of all sums), rgb8[c] its byte through the
// scene's thresholds, hits = min(hit_frames, 255).  n_frames <= 65,536 converts exactly.
RTX_HOST_DEVICE inline RtxPixelShade accum_resolve_statement(const float *thr, uint32_t n_frames, const RtxAccumPixel &acc)
{
    RtxPixelShade out;
    const float n = static_cast<float>(n_frames);
    for (int c = 0; c < 3; ++c) {
        out.linear[c] = acc.sum[c] / n;
        out.rgb8[c] = static_cast<uint8_t>(quantise_statement(thr, out.linear[c]));
    }
    out.hits = static_cast<uint8_t>(acc.hit_frames < 255u ? acc.hit_frames : 255u);
    return out;
}
constexpr uint32_t kMaxMeanFrames = 65536u;
// The adaptive mean of N frames (rtx_render_view_adaptive, rtx_moment_*_device; the kernels: rtx_adapt.hip).  Four
// statements, each one text for both compilers: rtxh_moment_add / rtxh_moment_resolve on the host, rtxe::moment_add_kernel /
// rtxe::moment_resolve_kernel and the masked view launch on the device.
// moment_add_statement: accum_add_statement's sum and hit_frames, word for word, beside the ordered f32 sum of the squares
// and the pixel's own frame count.  The square is a product rounded to f32 BEFORE it is added (two statements, and
// -ffp-contract=off on both sides: never an FMA).  first: what *m held is not read and may be anything.
RTX_HOST_DEVICE inline void moment_add_statement(bool first, const RtxPixelShade &shade, RtxMomentPixel *m)
{
    const uint32_t hit = shade.hits != 0 ? 1u : 0u;
    if (first) {
        __builtin_memcpy(m->sum, shade.linear, 12);
        for (int c = 0; c < 3; ++c) m->sumsq[c] = shade.linear[c] * shade.linear[c];
        m->hit_frames = hit;
        m->frames = 1u;
        return;
    }
    for (int c = 0; c < 3; ++c) {
        const float sq = shade.linear[c] * shade.linear[c];
        m->sum[c] = m->sum[c] + shade.linear[c];
        m->sumsq[c] = m->sumsq[c] + sq;
    }
    m->hit_frames = m->hit_frames + hit;
    m->frames = m->frames + 1u;
}
// moment_error_statement: the (biased) variance of the mean of the pixel's noisiest channel.  Per channel two correctly
// rounded divisions by (float)frames, a product rounded first, a subtraction, `v > 0 ? v : 0` — a NaN and a negative
// rounding residue both become +0 — and a third division; the maximum by `a < b ? b : a`.  Never NaN, never negative.
// frames <= 2^24 converts exactly.
RTX_HOST_DEVICE inline float moment_error_statement(const RtxMomentPixel &m)
{
    const float fn = static_cast<float>(m.frames);
    float e[3];
    for (int c = 0; c < 3; ++c) {
        const float mean = m.sum[c] / fn;
        const float q = m.sumsq[c] / fn;
        const float sq = mean * mean;
        float v = q - sq;
        v = v > 0.0f ? v : 0.0f;
        e[c] = v / fn;
    }
    const float worst = e[0] < e[1] ? e[1] : e[0];
    return worst < e[2] ? e[2] : worst;
}
// tile_stopped: the one predicate the masked view launch and the add both evaluate from a tile's 8-byte state; there is no
// separate "stopped" word.  A stopped tile's state is no longer written, so within a call stopping is final.
RTX_HOST_DEVICE inline bool tile_stopped(const RtxAdaptRule &rule, const RtxTileState &state)
{
    return state.frames >= rule.min_frames && state.err <= rule.max_variance;
}
// a rule a call accepts: min_frames >= 1, max_variance >= 0 (+infinity included; a NaN fails the comparison)
inline bool adapt_rule_ok(const RtxAdaptRule *rule) { return rule && rule->min_frames != 0u && rule->max_variance >= 0.0f; }
// moment_resolve_statement: accum_resolve_statement with the pixel's OWN frame count as the divisor.
RTX_HOST_DEVICE inline RtxPixelShade moment_resolve_statement(const float *thr, const RtxMomentPixel &m)
{
    RtxPixelShade out;
    const float n = static_cast<float>(m.frames);
    for (int c = 0; c < 3; ++c) {
        out.linear[c] = m.sum[c] / n;
        out.rgb8[c] = static_cast<uint8_t>(quantise_statement(thr, out.linear[c]));
    }
    out.hits = static_cast<uint8_t>(m.hit_frames < 255u ? m.hit_frames : 255u);
    return out;
}
// Where the host reads a sample table: the caller's n interleaved pairs, or — table == NULL — the seeded table of n pairs,
// whose entries sample_statement gives.  The accessor of every host reader (light_points_of and through it the lit calls'
// margin): a seeded table is never made on the host.
struct SampleSource {
    const float *table;
    uint64_t seed;
    uint32_t n;
    void pair(uint64_t k, float *u, float *v) const
    {
        if (table) { *u = table[2 * k]; *v = table[2 * k + 1]; return; }
        *u = sample_statement(seed, 2 * k);
        *v = sample_statement(seed, 2 * k + 1);
    }
};
// a call's light may have at most this many points (nb_ray x its sample count): rtx_*_lit, rtx_scene_light_points_for
constexpr uint64_t kMaxCallLightPoints = 1ull << 20;
// Triangle::new + get_bounding_box — triangle.rs:22-34, :45-56: e1 = v1 - v0, e2 = v2 - v0, normal = unit(cross(e1, e2))
// (nalgebra's dot: the accumulator starts at zero, x, y, z in turn; Unit::new_normalize: each component divided by the
// square root), the box by min_float / max_float (`a < b ? a : b`, `a < b ? b : a`, triangle.rs:37-43).  One text for both
// compilers, as light_sample_point is: triangle_derive (scene_prep.cpp) on the host, rtxp::pose_records_kernel
// (rtx_pose.hip) on the device, the same bits with -ffp-contract=off and the correctly rounded divide and square root.
RTX_HOST_DEVICE inline void triangle_statement(const float v0[3], const float v1[3], const float v2[3], float e1[3],
                                               float e2[3], float normal[3], float bmin[3], float bmax[3])
{
    for (int k = 0; k < 3; ++k) {
        e1[k] = v1[k] - v0[k];
        e2[k] = v2[k] - v0[k];
    }
    const float cx = e1[1] * e2[2] - e1[2] * e2[1];
    const float cy = e1[2] * e2[0] - e1[0] * e2[2];
    const float cz = e1[0] * e2[1] - e1[1] * e2[0];
    float acc = 0.0f;
    acc = acc + cx * cx;
    acc = acc + cy * cy;
    acc = acc + cz * cz;
    const float n = sqrtf(acc);
    normal[0] = cx / n;
    normal[1] = cy / n;
    normal[2] = cz / n;
    for (int k = 0; k < 3; ++k) {
        const float lo = v0[k] < v1[k] ? v0[k] : v1[k];
        const float hi = v0[k] < v1[k] ? v1[k] : v0[k];
        bmin[k] = lo < v2[k] ? lo : v2[k];
        bmax[k] = hi < v2[k] ? v2[k] : hi;
    }
}

// One node of the threaded (pre-order, skip-linked) BVH stream: 8 dwords, fetched
// by the kernel with one scalar 32-byte load.
//   inner node : info = index of its second child (< 2^30; its first child is at index+1; the reference-tree stream
//                leaves 0 here), link = index of the node to continue with when the subtree is skipped
//   leaf  node : info = 0x80000000|s, link = number of primitive records, s = first record;
//                bit 30 (kSphereFlag) set when the records are spheres — a leaf holds one arm of
//                Primitive only (src/tracer/primitives/mod.rs:40-43), so the kernel's dispatch on
//                the arm is a scalar branch per leaf
struct NodeRec {
    float    bmin[3];
    uint32_t link;
    float    bmax[3];
    uint32_t info;
};
static_assert(sizeof(NodeRec) == 32, "NodeRec must be 32 bytes");
// The same eight dwords in the order the kernel fetches them.  The multiply-based box test is three packed
// fused multiply-adds (v_pk_fma_f32: two planes per instruction), whose scalar operands must be adjacent
// registers of the 32-byte scalar load: (lo.x, lo.y), (hi.x, hi.y), (lo.z, hi.z).
struct NodeDev {
    float    lox, loy, hix, hiy, loz, hiz;
    uint32_t link, info;
};
static_assert(sizeof(NodeDev) == sizeof(NodeRec), "NodeDev is a permutation of NodeRec");
// inflate > 0: every plane is moved outwards by that much (PreparedScene::cull_delta) — the library's own stream only,
// whose boxes cull and nothing else; the reference-tree stream must stay exact.
inline std::vector<NodeDev> nodes_in_device_order(const std::vector<NodeRec> &v, float inflate = 0.0f)
{
    std::vector<NodeDev> out(v.size());
    for (size_t i = 0; i < v.size(); ++i)
        out[i] = NodeDev{v[i].bmin[0] - inflate, v[i].bmin[1] - inflate, v[i].bmax[0] + inflate, v[i].bmax[1] + inflate,
                         v[i].bmin[2] - inflate, v[i].bmax[2] + inflate, v[i].link, v[i].info};
    return out;
}
constexpr uint32_t kLeafFlag = 0x80000000u;
constexpr uint32_t kSphereFlag = 0x40000000u;
constexpr uint32_t kLeafIndexMask = 0x3FFFFFFFu;

// One triangle as the traversal consumes it: 16 dwords, one scalar 64-byte load.
// v0,e1,e2 are the 36 bytes Möller–Trumbore reads (triangle.rs:66-94); bmin/bmax are the
// triangle's own AABB (triangle.rs:45-56), needed because the reference only counts a leaf
// whose box test passed (bounding_volume_hierarchy.rs:52); idx = index in the caller's order.
// A Sphere (sphere.rs:12-18) uses the same 64-byte slot: v0 = origin, e1[0] = radius2 (sphere.rs:26),
// e1[1] = radius, bmin/bmax = origin -+ radius (sphere.rs:32-41); the leaf's kSphereFlag says which.
struct TriRec {
    float    v0[3];
    float    e1[3];
    float    e2[3];
    float    bmin[3];
    float    bmax[3];
    uint32_t idx;
};
static_assert(sizeof(TriRec) == 64, "TriRec must be 64 bytes");

// The f32 after x towards +infinity, for x >= +0.0: one more in the bit pattern (nextafterf there, which host and device
// cannot state differently: +0.0 gives the smallest subnormal); +infinity and a NaN come back as they are.
RTX_HOST_DEVICE inline float f32_successor(float x)
{
    if (!(x < __builtin_inff())) return x;
    uint32_t bits;
    __builtin_memcpy(&bits, &x, 4);
    ++bits;
    __builtin_memcpy(&x, &bits, 4);
    return x;
}
// Plane data of a global triangle (PreparedScene::global_planes; rtx_traverse.hpp: plane_rules_out) from its primitive
// record: v0 = v0, e1 = N, e2 = W, bmin[0] = K_d, idx = idx, every other word zero.  N and W in double from the f32 edges
// (the products of two f32 are exact there, so a fused form gives the same bits), N rounded to nearest, W upwards;
// K_d = 2^-19 * 2 * (Wx + Wy + Wz) + 2^-100 over the ROUNDED W in double, upwards.  Anything not comfortably finite
// switches the shortcut off for that triangle (K_d = inf).  One text for both compilers, as triangle_statement is:
// prepare_scene on the host, rtxg::global_planes_kernel (rtx_planes.hip) on the device for a pose's triangles.
RTX_HOST_DEVICE inline void global_plane_statement(const TriRec &t, TriRec *out)
{
    TriRec g = {};
    const double e1[3] = {t.e1[0], t.e1[1], t.e1[2]}, e2[3] = {t.e2[0], t.e2[1], t.e2[2]};
    double sum_w = 0.0;
    bool fine = true;
    for (int a = 0; a < 3; ++a) {
        const int b = (a + 1) % 3, c = (a + 2) % 3;
        const double n = e1[b] * e2[c] - e1[c] * e2[b];
        const double w = fabs(e1[b] * e2[c]) + fabs(e1[c] * e2[b]);
        g.v0[a] = t.v0[a];
        g.e1[a] = static_cast<float>(n);
        g.e2[a] = f32_successor(static_cast<float>(w));
        fine = fine && w < 0x1p100;                    // (false for a NaN and for infinity)
        sum_w += static_cast<double>(g.e2[a]);
    }
    const double kd = 0x1p-19 * 2.0 * sum_w + 0x1p-100;
    g.bmin[0] = fine ? f32_successor(static_cast<float>(kd)) : __builtin_inff();
    g.idx = t.idx;
    *out = g;
}

// Sphere::new + get_bounding_box — sphere.rs:21-41 — from s = {origin x, y, z, radius}: v0 = the origin, e1[0] = radius *
// radius, e1[1] = radius, the box = origin -+ radius (each word rounded once), and the origin once more for the shading
// record's `normal` words (get_normal needs p_hit, sphere.rs:93-95).  Every other word of the 64-byte slot stays what the
// caller holds there (zero in a prepared record).  One text for both compilers, as triangle_statement is: prepare_scene on
// the host, rtxm::overlay_kernel (rtx_prims.hip) on the device for a pose's spheres.
RTX_HOST_DEVICE inline void sphere_statement(const float s[4], float v0[3], float e1[3], float bmin[3], float bmax[3],
                                             float origin_for_shade[3])
{
    const float radius = s[3];
    e1[0] = radius * radius;
    e1[1] = radius;
    for (int k = 0; k < 3; ++k) {
        v0[k] = s[k];
        bmin[k] = s[k] - radius;
        bmax[k] = s[k] + radius;
        origin_for_shade[k] = s[k];
    }
}

// A pose made from the scene's vertices as created and a set of affine maps (rtx_scene_pose_moved; the kernel:
// rtx_move.hip).  A move is 12 floats, a 3 x 4 map, row major: the three words of a row of A, then the row's translation.
// One statement for a vertex (sphere = false: 3 words in, 3 out) and for a sphere's {origin x, y, z, radius} (sphere = true:
// 4 words): under move g, out[r] = ((m[4r] * p0 + m[4r+1] * p1) + m[4r+2] * p2) + m[4r+3] — three products and three sums in
// this order, each rounded to f32 once (both compilers run it under -ffp-contract=off) — and a sphere's radius times
// radius_scale[g], one product, or copied where radius_scale is NULL.  g == kMoveNone, and any other g that is not below
// n_moves, copies the words as they are: neither `moves` nor `radius_scale` is indexed with a value that has not been
// compared against n_moves.  The copy keeps the sign of a -0.0, which the identity matrix does not (-0.0 + 0.0 = +0.0).
// One text for both compilers, as triangle_statement and sphere_statement are: moved_prims on the host,
// rtxf::move_kernel on the device.
constexpr uint32_t kMoveNone = 0xFFFFFFFFu;
constexpr uint32_t kMaxMoves = 65536u;
RTX_HOST_DEVICE inline void move_statement(const float *moves, const float *radius_scale, uint32_t n_moves, uint32_t g,
                                           bool sphere, const float *in, float *out)
{
    if (g >= n_moves) {
        for (int k = 0; k < (sphere ? 4 : 3); ++k) out[k] = in[k];
        return;
    }
    const float *m = moves + 12u * static_cast<size_t>(g);
    for (int r = 0; r < 3; ++r) out[r] = ((m[4 * r] * in[0] + m[4 * r + 1] * in[1]) + m[4 * r + 2] * in[2]) + m[4 * r + 3];
    if (sphere) out[3] = radius_scale ? in[3] * radius_scale[g] : in[3];
}
// A skinned pose's corner (rtx_scene_pose_skinned; the kernel: rtx_skin.hip): the rest position `in` under up to four
// moves, blended.  All four bones not below n_moves (kMoveNone is such a value): the words are copied, no arithmetic, so a
// -0.0 keeps its sign.  Otherwise q_k = move_statement of slot k's bone — a bone not below n_moves gives `in` itself, by that
// statement's own rule, so `moves` is never indexed with a value that has not been compared against n_moves — and
// out[r] = ((w0 * q0[r] + w1 * q1[r]) + w2 * q2[r]) + w3 * q3[r]: four products and three sums in this order, each rounded
// to f32 once.  The weights are taken as given.  One text for both compilers, as move_statement is: skinned_prims on the
// host, rtxk::skin_kernel on the device.
RTX_HOST_DEVICE inline void skin_statement(const float *moves, uint32_t n_moves, const uint32_t bones[4], const float weights[4],
                                           const float in[3], float out[3])
{
    if (bones[0] >= n_moves && bones[1] >= n_moves && bones[2] >= n_moves && bones[3] >= n_moves) {
        for (int k = 0; k < 3; ++k) out[k] = in[k];
        return;
    }
    float q[4][3];
    for (int k = 0; k < 4; ++k) move_statement(moves, nullptr, n_moves, bones[k], false, in, q[k]);
    for (int r = 0; r < 3; ++r)
        out[r] = ((weights[0] * q[0][r] + weights[1] * q[1][r]) + weights[2] * q[2][r]) + weights[3] * q[3][r];
}

// Shading data of a primitive, indexed by its position in the caller's Vec<Primitive> (read once per hit).
struct ShadeRec {
    float    normal[3];   // triangle: Triangle::new, triangle.rs:29; sphere: its origin (normal = normalize(p_hit - origin), sphere.rs:93-95)
    uint32_t rank;        // tie rank (see RtxSceneDesc.tie_rank)
    float    rgb[3];      // Color
    uint32_t kind;        // 0 triangle, 1 sphere
};
static_assert(sizeof(ShadeRec) == 32, "ShadeRec must be 32 bytes");

struct PreparedScene {
    uint32_t width = 0, height = 0;
    float eye[3], cam_u[3], cam_v[3], cam_w[3];
    float distance = 0;
    uint32_t nb_ray = 1, nb_light_sample = 0;
    uint32_t n_tris = 0;               // primitives in the Vec (both arms)
    uint32_t n_spheres = 0;            // of which spheres
    uint32_t n_samples = 0;
    std::vector<NodeRec>  nodes;
    // The same tree as a second stream for the PRIMARY rays (probe_kernel), of every node's two children the one whose box
    // centre lies nearer the EYE first (made while the closest-hit walks pruned by the closest hit so far; they no longer do,
    // rtx_traverse.hpp: advance_to_leaf, and visit the same records in either order); `nodes` puts the child farther from
    // the LIGHT first, which is what the shadow walks want.  Same records,
    // same leaves (a leaf names its run of the primitive array), other order and links.  Empty: `nodes` serves both.
    std::vector<NodeRec>  primary_nodes;
    std::vector<NodeRec>  ref_nodes;   // the reference's own tree as a stream (empty when not built)
    std::vector<TriRec>   tris;        // primitive records (triangles and spheres) in leaf order
    std::vector<ShadeRec> shade;       // in caller order
    std::vector<float>    samples;     // n_samples x 2; empty while the table is a seeded one (rtx_scene_reseed)
    // The table as it stands (resample_scene): seeded, its n_samples entries are sample_statement's over sample_seed and no
    // array holds them on the host (sample_source is how the host reads either kind).  table_generation counts the accepted
    // replacements, so that a device knows the table, the light arrays and the margin it holds are stale.
    bool     seeded = false;
    uint64_t sample_seed = 0;
    uint64_t table_generation = 0;
    float light_v[9];                // the light triangle as given: v0, v1, v2 (rtx_scene_light)
    std::vector<float>    light_points;// nb_ray x nb_light_sample x 3
    // The same points in the order the shading pass WALKS them: per primary ray and per batch of kMaxLightBatch
    // consecutive samples a short tour that starts at the batch's first sample (light_tour_order).  One 16-byte record
    // per walk position, at the position's place in its batch: x, y, z and — as bits, not a value — the sample's index
    // WITHIN the batch, the column its result belongs to.  light_order: the same order as sample indices
    // (r, batch after batch: the index within nb_light_sample at each walk position).
    std::vector<float>    light_tour;  // nb_ray x nb_light_sample x 4
    std::vector<uint32_t> light_order; // nb_ray x nb_light_sample
    float gamma_thr[256];
    uint32_t n_leaves = 0, max_leaf_tris = 0, depth = 0;
    // Outward shift of the culling planes on the device, 2^-19 x the largest coordinate magnitude of the scene and the
    // eye: it absorbs the error of the multiply-based plane distances (at most 11.01 * 2^-24 of that magnitude in
    // position units, rtx_traverse.hpp), so that the box test needs no per-test widening.
    float cull_delta = 0.0f;
    // per primary ray r: bounding box of its light points (lo xyz, hi xyz), and the margin of the tile shaft test,
    // 2^-16 x the largest coordinate magnitude of scene, eye and light points (rtx_pass_schedule.hpp: shaft_cut)
    std::vector<float>    light_boxes;
    float shaft_delta = 0.0f;
    // what shaft_delta is folded from beside the light boxes: the largest coordinate magnitude of the scene and the eye
    // (shaft_delta_of; a call's light folds its own boxes onto it)
    float scene_magnitude = 0.0f;
    uint32_t leaf_max = 4;   // records a leaf of a tree built for this scene may hold (RtxSceneDesc.leaf_max, 0: 4)
    uint32_t n_global = 0;   // > 0: records [0, n_global) are the "global" triangles, stream = root, their leaf, the tree proper
    // one per global triangle, in TriRec clothing: v0 = v0, e1 = fl(e1 x e2), e2 = (|e1| x |e2| with plus signs, rounded
    // up), bmin[0] = the denominator's error allowance — what rtx_traverse.hpp: plane_rules_out needs
    std::vector<TriRec>   global_planes;
    // The scheduling pass's prediction of the long primary walks (predict_long_tiles): the 8 x 8 pixel tiles of the
    // scene's own frame, numbered row-major (tile_y * tiles_x + tile_x), whose predicted primary walk weighs at least
    // kProbeLongWeight — costliest first, at most probe_long_cap of them — their weights, and a bit per frame tile
    // (word t / 32, bit t % 32) that is set for the listed ones.  An ordering hint: it never decides a pixel.  All
    // three are empty for a scene that does not cut per tile (more than kProbeSplitMaxNodes records) or whose camera or
    // sample table gives no proper frustum.
    std::vector<uint32_t> long_tiles, long_weights, long_bits;
    // range of the two columns of the sample table the scene was CREATED with (NaN: not finite); like the prediction made
    // from it, kept as created when the table is replaced
    float sample_lo[2] = {0.0f, 0.0f}, sample_hi[2] = {0.0f, 0.0f};
    // The "rest" geometry of rtx_scene_pose_moved: RtxSceneDesc.v0v1v2 and .spheres as given (a primitive record keeps v0,
    // e1 and e2, from which v1 and v2 cannot be had exactly), and for every triangle and every sphere its position in the
    // Vec, where a pose's `group` array names its move.  No record, stream or table above is made from them.
    std::vector<float>    rest_v0v1v2, rest_spheres;     // n_triangles x 9, n_spheres x 4
    std::vector<uint32_t> rest_tri_vec, rest_sphere_vec; // n_triangles, n_spheres
};
// A tile is long when the records its frustum meets weigh at least this much (an inner record 1, a leaf 1 + 3 x its
// primitive records: the proxy of rtx_pass_schedule.hpp's cut).  Chosen by measurement (the
// weight follows a tile's measured primary walk with a correlation of 0.985; swept over 150 ... 400, the scheduling pass is
// shortest at 300, where a 1080p frame of the default scene lists its 52 costliest tiles).
#ifndef RTX_PROBE_LONG_WEIGHT
#define RTX_PROBE_LONG_WEIGHT 300
#endif
constexpr uint32_t kProbeLongWeight = RTX_PROBE_LONG_WEIGHT;
// scenes of more stream records do not cut per tile (rtx_device.h: kCutMaxNodes, the same number) and predict nothing
constexpr uint32_t kProbeSplitMaxNodes = 1u << 16;
// A list of fewer tiles is dropped.  Such a scene's tail is not a dozen silhouette tiles but the whole mesh in a tile or two
// (the small bunny in a 1080p frame: 2 tiles of weight 18,399), where each of the four beams still meets all of it: measured
// with the list +2 % on that frame's pass (profiles/r08/e_ab_without_a_list.log, C2).
constexpr uint32_t kProbeLongMinTiles = 8u;
inline uint32_t probe_long_cap(uint32_t n_tiles) { return n_tiles / 32u < 1024u ? n_tiles / 32u : 1024u; }
// Weight of the primary-stream records whose stored box (planes moved outwards by cull_delta, as uploaded) meets the
// frustum of frame tile (tile_x, tile_y): the eye and the tile's pixel rectangle, widened by the sample table's range
// and one more pixel on each side.  A superset count: a record that any primary ray of the tile can pass is met.  The
// tree proper only (the root and the global triangles' leaf, which every walk takes untested, weigh nothing and count as
// met).  met: NULL, or one byte per record of the stream, set to 1 for the records met.  *valid = false (and 0): no
// prediction for this scene.
uint32_t probe_tile_weight(const PreparedScene &s, uint32_t tile_x, uint32_t tile_y, uint8_t *met, bool *valid);
// fills long_tiles, long_weights and long_bits for `threshold` (prepare_scene: kProbeLongWeight).  Weighs every tile of the
// frame, also of a frame whose full launch is too large for the list (rtx_device.h: kProbeSplitMaxTiles): a share of its rows
// is not.  A tile beside the mesh ends at the first records, so the cost follows the mesh more than the frame: measured on
// the host 0.03 s of a scene creation of 0.11 s (big_bunny, 1920 x 1080) and of 0.13 s (4096 x 4096).
void predict_long_tiles(PreparedScene &s, uint32_t threshold);
constexpr uint32_t kMaxGlobalPrims = 8u;
// the walk addresses primitive records by 32-bit byte offsets, 64 B each
constexpr uint64_t kMaxPrimitives = 1ull << 26;

// Light samples per LDS batch of the shading pass (results of one batch: 64 pixels x batch floats).
#ifndef RTX_LIGHT_BATCH
#define RTX_LIGHT_BATCH 128
#endif
constexpr uint32_t kMaxLightBatch = RTX_LIGHT_BATCH;

// Order of walking n points (xyz, f32): order[0] = 0, then nearest neighbour (Euclidean, in double, ties to the lower
// index), then 2-opt reversals that keep position 0, a bounded number of passes.  Always a permutation of 0 .. n-1: a
// distance that is NaN or infinite never wins a comparison.  Deterministic.
void light_tour_order(const float *points, uint32_t n, uint32_t *order);

// The tour of a light given per call (rtx_render_view_rows_lit): light_tour_order's scan in f32 — distances by
// tour_distance, `before` and `after` each an f32 sum of two of them — so that the device can make it word for word
// (rtxt::tour_kernel).  A statement of its own: a created scene's tour stays light_tour_order's.  Always a permutation of
// 0 .. n-1 that starts with 0, whatever the points hold.
void light_tour_order_f32(const float *points, uint32_t n, uint32_t *order);
// per primary ray r < nb_ray the bounding box (lo xyz, hi xyz) of its nb_light points, fmin / fmax from -+infinity (a NaN
// is ignored): PreparedScene::light_boxes.  out: nb_ray x 6.
void light_boxes_of(const float *points, uint32_t nb_ray, uint32_t nb_light, float *out);
// PreparedScene::shaft_delta from PreparedScene::scene_magnitude and n light-box bounds (the finite ones count)
float shaft_delta_of(float scene_magnitude, const float *light_boxes, size_t n);

// Returns RTX_OK or a negative RtxError.
int prepare_scene(const RtxSceneDesc &desc, PreparedScene &out);

// `nodes` (pre-order, inner.info = second child) with the children of every inner node below record `root` in the order
// that puts the one nearer to `point` first; records before `root` are kept as they are.
void stream_nearest_first(const std::vector<NodeRec> &nodes, uint32_t root, const float *point, std::vector<NodeRec> &out);

// ---- pieces with their own tests ----
void camera_new(const float eye[3], const float look_at[3], const float up[3],
                float u[3], float v[3], float w[3]);
void triangle_derive(const float v0[3], const float v1[3], const float v2[3],
                     float e1[3], float e2[3], float normal[3], float bmin[3], float bmax[3]);
void light_sample(const float v0[3], const float v1[3], const float v2[3], float u, float v, float out[3]);
// out[3 * (r * nb_light + i)] = light_sample(tri, T[(r * nb_ray + i) % n_samples]) for r < nb_ray, i < nb_light
// (main.rs:194-196; T: the table `samples` reads, n != 0): a scene's light points, and any other light's on it
void light_points_of(const float tri[9], const SampleSource &samples, uint32_t nb_ray, uint32_t nb_light, float *out);
// the scene's table as it stands, for a host reader
inline SampleSource sample_source(const PreparedScene &s)
{
    return SampleSource{s.seeded ? nullptr : s.samples.data(), s.sample_seed, s.n_samples};
}
// What a scene derives from its sample table (prepare_scene, resample_scene — the one statement of both): the light points,
// their tour per primary ray and batch (light_tour, light_order: PreparedScene's) and the light boxes.  The shaft margin is
// shaft_delta_of over the boxes.  May throw std::bad_alloc.
void light_walk_of(const float tri[9], const SampleSource &samples, uint32_t nb_ray, uint32_t nb_light,
                   std::vector<float> &points, std::vector<float> &tour, std::vector<uint32_t> &order,
                   std::vector<float> &boxes);
// What the render pipeline reads of a light over a sample table beside its points, as the host states it (a lit pipeline
// call's light over the scene's table; a frame of rtx_render_view_rows_mean: `tri` with `count` samples over the SEEDED table
// samples = {NULL, seed, n_pairs}, in closed form over the nb_ray * count entries the points read — no table is made):
// order, nb_ray x count sample indices, the tour per primary ray and batch in rtx_scene_light_order's form; boxes, nb_ray x 6;
// shaft_delta, shaft_delta_of over those boxes.  Each output may be NULL.  O(nb_ray * count) for the margin alone; the tour
// costs what light_tour_order_f32 costs.  May throw std::bad_alloc.
void light_walk_statement(const PreparedScene &p, const float tri[9], uint32_t count, const SampleSource &samples, uint32_t *order,
                          float *boxes, float *shaft_delta);
// Replaces the scene's table by `samples` (rtx_scene_resample: a caller's table, copied; rtx_scene_reseed: table == NULL)
// and re-derives what prepare_scene derives from it, by light_walk_of and shaft_delta_of.  RTX_ERR_BAD_ARG: n == 0;
// RTX_ERR_UNSUPPORTED: the margin is not finite (prepare_scene's rule); RTX_ERR_OOM.  On an error the scene is as it was;
// accepted, table_generation advances.  The prediction of the long walks and sample_lo / sample_hi stay as created.  A
// seeded table costs work proportional to nb_ray * nb_light_sample and none proportional to n.
int resample_scene(PreparedScene &s, const SampleSource &samples);
// byte = (x.powf(1/2.2) * 255.0) as u8 with the host libm — color.rs:10-13,28-33
uint8_t gamma_quantise(float linear);
int  build_gamma_thresholds(float thr[256]);
int  ref_leaf_rank(uint32_t n_tris, const float *v0v1v2, uint32_t *out_rank);
int  ref_tree_build(uint32_t n_tris, const float *v0v1v2, uint32_t *out_rank, std::vector<NodeRec> *out_stream);
// same over the primitives' own boxes (n x {min xyz, max xyz}) — what the reference clusters by, whatever the arm
int  ref_tree_build_boxes(uint32_t n, const float *lo_hi, uint32_t *out_rank, std::vector<NodeRec> *out_stream);
// above this many primitives RTX_REFTREE_AUTO skips the O(n^2) reference tree (the reference itself could not build it)
constexpr uint32_t kRefTreeAutoMax = 50000u;

// ---- posing an uploaded scene's triangles (rtx_scene_pose; the kernels: rtx_pose.hip) ----
// A pose is n_tris x 9 floats in RtxSceneDesc.v0v1v2's layout: the Vec's triangles in Vec order, spheres skipped (they
// move through a PrimsOverlay, below).  The tree keeps its shape: every record of `nodes` holds the exact union of the primitives' own boxes over a
// contiguous run of the primitive array (TreeBuilder::build, the global leaf, the root over all, both RTX_ACCEL_BRUTE
// shapes), so record i's posed box is a min/max fold over records [first_i, first_i + count_i), independent of every
// other node.  The refit kernels fold each range directly, a range of at most kPoseLaneMax records by one work-item and a
// longer one by one workgroup of kPoseBlock work-items: `order` lists the nodes, the n_long long ranges first.
constexpr uint32_t kPoseLaneMax = 32u;
constexpr uint32_t kPoseBlock = 256u;
constexpr uint32_t kPoseNoTriangle = 0xFFFFFFFFu;
struct PoseTables {
    std::vector<uint32_t> ranges;      // n_nodes x {first, count}
    std::vector<uint32_t> tri_of;      // Vec position -> triangle number in the pose; a sphere: kPoseNoTriangle
    std::vector<uint32_t> sphere_of;   // Vec position -> sphere number (rtx_scene_pose_prims); a triangle: kPoseNoTriangle
    std::vector<uint32_t> order;       // the nodes: those with count > kPoseLaneMax (ascending), then the others (ascending)
    uint32_t n_long = 0;
};
void pose_tables(const PreparedScene &s, PoseTables &out);
// what PreparedScene::cull_delta and origin_bound were sized for bounds the pose: every coordinate finite and of
// magnitude at most scene_magnitude
bool pose_in_range(const PreparedScene &s, const float *pose);
// What a pose states beside the triangles' vertices (rtx_scene_pose_prims; the kernel: rtx_prims.hip): each array is NULL,
// "as uploaded", or one entry per primitive of its arm in Vec order — spheres: n_spheres x {origin x, y, z, radius};
// rgb: n_triangles x 3; sphere_rgb: n_spheres x 3.
struct PrimsOverlay {
    const float *spheres = nullptr, *rgb = nullptr, *sphere_rgb = nullptr;
    bool any() const { return spheres || rgb || sphere_rgb; }
};
// The host statement of rtxm::overlay_kernel: the uploaded primitive records (leaf order) and shading records (Vec order)
// with every sphere restated by sphere_statement and every rgb replaced where `ov` gives one, every other word copied.
// They stand where the uploaded arrays stand for posed_records and rebuilt_records.  Each output may be NULL.
void overlay_records(const PreparedScene &s, const PoseTables &t, const PrimsOverlay &ov, TriRec *tris, ShadeRec *shade);
// pose_in_range's rule for posed spheres: all four values finite, and the six box words origin -+ radius, as
// sphere_statement rounds them, of magnitude at most scene_magnitude
bool spheres_in_range(const PreparedScene &s, const float *spheres);
// What a moved pose states (rtx_scene_pose_moved): n_moves maps of 12 floats, the move each Vec position follows (group:
// NULL, every primitive follows move 0; kMoveNone: none) and a factor per move for a sphere's radius (NULL: radii as
// created).  moved_prims is the host statement of rtxf::move_kernel: move_statement over the rest geometry, into the
// arrays rtx_scene_pose_prims is then handed as v0v1v2 (n_triangles x 9) and spheres (n_spheres x 4).  Either may be NULL.
struct PoseMoves {
    uint32_t n_moves = 0;
    const float *moves = nullptr;
    const uint32_t *group = nullptr;
    const float *radius_scale = nullptr;
};
void moved_prims(const PreparedScene &s, const PoseMoves &m, float *out_v0v1v2, float *out_spheres);
// pose_in_range and spheres_in_range over moved_prims' output, stated without making it: the statement runs once more per
// vertex and sphere, and nothing is stored (a moved pose's host call touches no array of the pose's size but `group`)
bool moved_in_range(const PreparedScene &s, const PoseMoves &m);
// the host variant's rule for `group`: every entry below n_moves or kMoveNone (true for a NULL array)
bool move_groups_ok(const PreparedScene &s, const PoseMoves &m);
// The skin of a scene (rtx_scene_skin): per triangle corner four bones and four weights — corner c of triangle t at
// [12 t + 4 c, 12 t + 4 c + 4), the order of rest_v0v1v2's vertices — and per sphere one bone; 96 bytes per triangle and 4 per
// sphere of host memory.  max_bone: the largest bone other than kMoveNone over both arrays (0: none).  generation: counts the
// binds and unbinds of the scene, so that a device knows its copy is stale.
struct Skin {
    std::vector<uint32_t> bones;        // n_triangles x 12
    std::vector<float>    weights;      // n_triangles x 12
    std::vector<uint32_t> sphere_bone;  // n_spheres (kMoveNone where the bind gave no array)
    uint32_t max_bone = 0;
    bool bound = false;
    uint64_t generation = 0;
};
// Copies the caller's arrays into `out` for scene `s` (sphere_bone may be NULL).  RTX_ERR_BAD_ARG: NULL bones or weights with
// triangles present; RTX_ERR_UNSUPPORTED: a weight that is not finite; `out` is then left as it was.  RTX_ERR_OOM.
int skin_bind(const PreparedScene &s, const uint32_t *bones, const float *weights, const uint32_t *sphere_bone, Skin &out);
// The host statement of rtxk::skin_kernel: skin_statement over every corner of the rest geometry and move_statement over
// every sphere under sphere_bone, into moved_prims' two arrays (either may be NULL).  m.group is not read: the skin names
// the moves.  skinned_in_range: moved_in_range's rule over that output, stated without making it.
void skinned_prims(const PreparedScene &s, const Skin &skin, const PoseMoves &m, float *out_v0v1v2, float *out_spheres);
bool skinned_in_range(const PreparedScene &s, const Skin &skin, const PoseMoves &m);
// The host statement of what the pose kernels make.  rank: per Vec position, or NULL for the position itself.  tris:
// n_prims records in leaf order; shade: n_prims in Vec order; nodes: n_nodes records in NodeRec's word order, the planes
// moved outwards by cull_delta in f32 as nodes_in_device_order moves them.  Each output may be NULL.  ov: NULL, or what
// the pose states beside the vertices (overlay_records' words in place of the uploaded ones); pose may be NULL for a scene
// without triangles.
void posed_records(const PreparedScene &s, const PoseTables &t, const float *pose, const uint32_t *rank, TriRec *tris,
                   ShadeRec *shade, NodeRec *nodes, const PrimsOverlay *ov = nullptr);
// The reference's own tree over the posed primitives (ref_tree_build_boxes, O(n^2)): its leaf ranks per Vec position and
// its stream, the leaves naming positions of the primitive array as PreparedScene::ref_nodes' do.
int posed_ref_tree(const PreparedScene &s, const PoseTables &t, const float *pose, std::vector<uint32_t> &rank,
                   std::vector<NodeRec> &stream, const PrimsOverlay *ov = nullptr);


// ---- a pose whose tree is rebuilt (rtx_scene_pose_rebuilt; the kernels: rtx_rebuild.hip) ----
// The records of the tree proper — [n_global, n_prims) of the uploaded array — are sorted by a 64-bit key of their posed
// own boxes, and a balanced tree is laid over the sorted runs.  Its shape depends on n_global, the two run lengths and
// leaf_max alone, so every word of link / info, every node's (first, count) and the refit kernels' order are made once per
// scene (rebuild_tables); only the permutation, the records and the boxes (the refit kernels' fold) are per pose.
constexpr uint32_t kRebuildCellBits = 21u;
constexpr uint32_t kRebuildCellMax = (1u << kRebuildCellBits) - 1u;
// S of rebuild_key_statement for the pose bound M: 2^21 / (2 M), rounded to f32 once
inline float rebuild_key_scale(float bound) { return static_cast<float>(2097152.0 / (2.0 * static_cast<double>(bound))); }
// The key of a record from its own (posed) box: bit 63 the arm (1: sphere), bits 62..0 the Morton interleave of the cells
// of the box centre, x in the highest bit of every triple.  c = 0.5f * (bmin + bmax); cell = (uint32)((c + M) * S) held to
// [0, 2^21 - 1], a NaN to 0.  One text for both compilers, as triangle_statement is: rebuilt_records on the host,
// rtxb::key_kernel (rtx_rebuild.hip) on the device; two additions and two multiplications, each rounded once.
RTX_HOST_DEVICE inline uint64_t rebuild_key_statement(const float bmin[3], const float bmax[3], bool sphere, float bound,
                                                      float scale)
{
    uint64_t key = sphere ? 1ull << 63 : 0ull;
    for (int k = 0; k < 3; ++k) {
        const float c = 0.5f * (bmin[k] + bmax[k]);
        const float f = (c + bound) * scale;
        uint32_t q = 0u;                                   // (a NaN, and anything below the frame)
        if (f >= 2097151.0f) q = kRebuildCellMax;
        else if (f >= 0.0f) q = static_cast<uint32_t>(f);
        uint64_t x = q;                                    // 21 bits, two zeros between each
        x = (x | x << 32) & 0x1F00000000FFFFull;
        x = (x | x << 16) & 0x1F0000FF0000FFull;
        x = (x | x << 8) & 0x100F00F00F00F00Full;
        x = (x | x << 4) & 0x10C30C30C30C30C3ull;
        x = (x | x << 2) & 0x1249249249249249ull;
        key |= x << (2 - k);
    }
    return key;
}
struct RebuildTables {
    std::vector<NodeRec>  nodes;       // the rebuilt stream's link and info; the boxes are zero
    std::vector<uint32_t> ranges;      // n_nodes x {first, count}, positions of the SORTED primitive array
    std::vector<uint32_t> order;       // as PoseTables::order
    uint32_t n_long = 0;
    uint32_t n_tree_tris = 0, n_tree_spheres = 0;      // the two runs of the tree proper
};
void rebuild_tables(const PreparedScene &s, RebuildTables &out);
// The host statement of a rebuilt pose.  keys, perm: one per record of the tree proper, in sorted order; perm[p] is the
// position in the uploaded array of the record that sorted position n_global + p holds (std::stable_sort by key: equal
// keys keep uploaded order).  tris: n_prims records in sorted order; shade: n_prims in Vec order, as posed_records makes
// them; nodes: the rebuilt stream in NodeRec's word order, the planes moved outwards by cull_delta.  Each may be NULL.
// ov: as posed_records'.
void rebuilt_records(const PreparedScene &s, const PoseTables &t, const RebuildTables &b, const float *pose,
                     const uint32_t *rank, uint64_t *keys, uint32_t *perm, TriRec *tris, ShadeRec *shade, NodeRec *nodes,
                     const PrimsOverlay *ov = nullptr);
// posed_ref_tree with its leaves naming positions of the SORTED primitive array (perm: rebuilt_records')
int rebuilt_ref_tree(const PreparedScene &s, const PoseTables &t, const float *pose, const uint32_t *perm,
                     std::vector<uint32_t> &rank, std::vector<NodeRec> &stream, const PrimsOverlay *ov = nullptr);

}  // namespace rtx
