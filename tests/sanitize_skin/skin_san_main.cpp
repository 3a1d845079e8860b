// Sanitizer leg for the host statement of a skinned pose (never on the GPU): scene_prep.cpp and host_helpers.cpp are
// compiled with -fsanitize=address,undefined together with this driver, which pushes small scenes — spheres alone,
// triangles alone, every third primitive a sphere at 255, 256 and 257 primitives — through skin_bind, skinned_prims and
// skinned_in_range with NaN and infinite weights and moves, bones at, beyond and far beyond n_moves, RTX_MOVE_NONE in
// some and in all slots, a NULL sphere_bone and radius_scale NULL and given; a scene of no primitive at all (a
// PreparedScene as constructed) goes through the same.  The caller's bones, weights, sphere_bone, moves and radius_scale
// are allocated at their exact size, so a read behind a bind's arrays, or an index that was not compared against n_moves,
// is a heap overflow the sanitizer reports.  tests/test_skin_host.py builds and runs it; any report makes the process
// exit non-zero.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "../../include/rtx.h"
#include "../../ray-tracer-rust_amd/csrc/scene_prep.h"

static int fails = 0;
#define CHECK(c) do { if (!(c)) { std::fprintf(stderr, "CHECK failed %s:%d: %s\n", __FILE__, __LINE__, #c); ++fails; } } while (0)

static bool same(const void *a, const void *b, size_t bytes) { return bytes == 0 || std::memcmp(a, b, bytes) == 0; }

static const float kIdentity[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};

// the two statements once more, spelled out, for one point
static void point(const float *m, const float *p, float *out)
{
    for (int r = 0; r < 3; ++r) {
        const float a = m[4 * r] * p[0], b = m[4 * r + 1] * p[1], c = m[4 * r + 2] * p[2];
        const float ab = a + b, abc = ab + c;
        out[r] = abc + m[4 * r + 3];
    }
}

static void corner(const float *moves, uint32_t n_moves, const uint32_t *b, const float *w, const float *p, float *out)
{
    if (b[0] >= n_moves && b[1] >= n_moves && b[2] >= n_moves && b[3] >= n_moves) {
        std::memcpy(out, p, 12);
        return;
    }
    float q[4][3];
    for (int k = 0; k < 4; ++k) {
        if (b[k] < n_moves) point(moves + 12 * static_cast<size_t>(b[k]), p, q[k]);
        else std::memcpy(q[k], p, 12);
    }
    for (int r = 0; r < 3; ++r) {
        const float x0 = w[0] * q[0][r], x1 = w[1] * q[1][r], x2 = w[2] * q[2][r], x3 = w[3] * q[3][r];
        const float s01 = x0 + x1, s012 = s01 + x2;
        out[r] = s012 + x3;
    }
}

static void through(const rtx::PreparedScene &s, uint32_t n_moves)
{
    const size_t nt = s.rest_tri_vec.size(), ns = s.rest_sphere_vec.size(), nc = 3 * nt;
    const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
    // exact-size arrays on the heap
    std::vector<float> moves(12 * static_cast<size_t>(n_moves)), scale(n_moves);
    for (uint32_t g = 0; g < n_moves; ++g) {
        std::memcpy(&moves[12 * static_cast<size_t>(g)], kIdentity, sizeof kIdentity);
        moves[12 * static_cast<size_t>(g) + 1] = 0.125f * float(g % 5);
        moves[12 * static_cast<size_t>(g) + 3] = 0.5f * float(g % 7) - 1.0f;
        moves[12 * static_cast<size_t>(g) + 11] = -0.25f * float(g % 3);
        scale[g] = 0.5f * float(g % 4);
    }
    // bones: in range, one slot NONE, all slots NONE, and values at, beyond and far beyond n_moves; weights a partition of one
    std::vector<uint32_t> bones(4 * nc), sphere_bone(ns);
    std::vector<float> weights(4 * nc);
    const uint32_t wild[4] = {n_moves, n_moves + 1u, 0xFFFFFFFEu, 0x80000000u};
    for (size_t c = 0; c < nc; ++c)
        for (size_t k = 0; k < 4; ++k) {
            uint32_t b = static_cast<uint32_t>((c + k) % n_moves);
            if (c % 5 == 4 && k == 2) b = rtx::kMoveNone;
            if (c % 7 == 3) b = rtx::kMoveNone;
            if (c % 11 == 6) b = wild[k];                       // a corner of nothing but bones out of range
            if (c % 13 == 2 && k == c % 4) b = wild[c % 3];     // one such slot beside followed ones
            bones[4 * c + k] = b;
            weights[4 * c + k] = 0.0625f * float(1 + (c + 3 * k) % 7);
        }
    for (size_t c = 0; c < nc; ++c) {
        const float sum = weights[4 * c] + weights[4 * c + 1] + weights[4 * c + 2] + weights[4 * c + 3];
        for (size_t k = 0; k < 4; ++k) weights[4 * c + k] /= sum;
    }
    for (size_t i = 0; i < ns; ++i) sphere_bone[i] = i % 4 == 3 ? rtx::kMoveNone : i % 9 == 5 ? wild[i % 4] : static_cast<uint32_t>(i % n_moves);
    rtx::Skin skin;
    CHECK(!skin.bound && skin.generation == 0);
    // what a bind refuses leaves the skin as it was
    if (nt) {
        CHECK(rtx::skin_bind(s, nullptr, weights.data(), nullptr, skin) == RTX_ERR_BAD_ARG);
        CHECK(rtx::skin_bind(s, bones.data(), nullptr, nullptr, skin) == RTX_ERR_BAD_ARG);
        for (float bad : {nan, inf, -inf})
            for (size_t at : {size_t(0), 2 * nc, 4 * nc - 1}) {
                std::vector<float> w2(weights);
                w2[at] = bad;
                CHECK(rtx::skin_bind(s, bones.data(), w2.data(), sphere_bone.data(), skin) == RTX_ERR_UNSUPPORTED);
            }
        CHECK(!skin.bound && skin.generation == 0);
    } else {
        CHECK(rtx::skin_bind(s, nullptr, nullptr, nullptr, skin) == RTX_OK && skin.bound && skin.generation == 1);      // nothing to read
        skin = rtx::Skin();
    }
    // NULL sphere_bone: every sphere stays; radius_scale NULL: radii copied
    CHECK(rtx::skin_bind(s, bones.data(), weights.data(), nullptr, skin) == RTX_OK && skin.bound && skin.generation == 1);
    CHECK(skin.bones.size() == 4 * nc && skin.weights.size() == 4 * nc && skin.sphere_bone.size() == ns);
    uint32_t top = 0;
    for (uint32_t b : bones)
        if (b != rtx::kMoveNone && b > top) top = b;
    CHECK(skin.max_bone == top);
    std::vector<float> v(9 * nt), sph(4 * ns), v2(9 * nt), sph2(4 * ns);
    rtx::PoseMoves m;
    m.n_moves = n_moves;
    m.moves = moves.data();
    rtx::skinned_prims(s, skin, m, v.data(), sph.data());
    for (size_t c = 0; c < nc; ++c) {
        float want[3];
        corner(moves.data(), n_moves, &bones[4 * c], &weights[4 * c], &s.rest_v0v1v2[3 * c], want);
        CHECK(same(want, &v[3 * c], 12));
        if (c % 7 == 3 || c % 11 == 6) CHECK(same(&v[3 * c], &s.rest_v0v1v2[3 * c], 12));
    }
    CHECK(same(sph.data(), s.rest_spheres.data(), 4 * sph.size()));
    rtx::skinned_prims(s, skin, m, nullptr, nullptr);      // either output may be NULL
    rtx::skinned_prims(s, skin, m, v2.data(), nullptr);
    rtx::skinned_prims(s, skin, m, nullptr, sph2.data());
    CHECK(same(v.data(), v2.data(), 4 * v.size()) && same(sph.data(), sph2.data(), 4 * sph.size()));
    // a second bind replaces the first: sphere_bone and radius_scale given
    CHECK(rtx::skin_bind(s, bones.data(), weights.data(), sphere_bone.data(), skin) == RTX_OK && skin.generation == 2);
    for (uint32_t b : sphere_bone)
        if (b != rtx::kMoveNone && b > top) top = b;
    CHECK(skin.max_bone == top);
    m.radius_scale = scale.data();
    rtx::skinned_prims(s, skin, m, v2.data(), sph.data());
    CHECK(same(v.data(), v2.data(), 4 * v.size()));
    for (size_t i = 0; i < ns; ++i) {
        const uint32_t g = sphere_bone[i];
        float want[4];
        std::memcpy(want, &s.rest_spheres[4 * i], 16);
        if (g < n_moves) {
            point(&moves[12 * static_cast<size_t>(g)], &s.rest_spheres[4 * i], want);
            want[3] = s.rest_spheres[4 * i + 3] * scale[g];
        }
        CHECK(same(want, &sph[4 * i], 16));
    }
    // the gentle moves and a partition of one stay within the bound, and the two rules agree
    CHECK(rtx::skinned_in_range(s, skin, m) == ((!nt || rtx::pose_in_range(s, v.data())) && (!ns || rtx::spheres_in_range(s, sph.data()))));
    // fewer moves than the skin names (the device variant's broken precondition): the statement reads no move beyond the count
    if (n_moves > 1) {
        const uint32_t fewer = n_moves / 2;
        std::vector<float> mv2(moves.begin(), moves.begin() + 12 * static_cast<size_t>(fewer)), sc2(scale.begin(), scale.begin() + fewer);
        rtx::PoseMoves m2;
        m2.n_moves = fewer;
        m2.moves = mv2.data();
        m2.radius_scale = sc2.data();
        rtx::skinned_prims(s, skin, m2, v2.data(), sph2.data());
        for (size_t c = 0; c < nc; ++c) {
            float want[3];
            corner(mv2.data(), fewer, &bones[4 * c], &weights[4 * c], &s.rest_v0v1v2[3 * c], want);
            CHECK(same(want, &v2[3 * c], 12));
        }
        (void)rtx::skinned_in_range(s, skin, m2);
    }
    // NaN and infinite entries of a move: the output leaves the range rule where the move is followed
    for (float w : {nan, inf, -inf})
        for (int at : {0, 3, 5, 10, 11}) {
            std::vector<float> mv2(moves);
            mv2[at] = w;
            rtx::PoseMoves m2 = m;
            m2.moves = mv2.data();
            rtx::skinned_prims(s, skin, m2, v2.data(), sph2.data());
            const bool fine = (!nt || rtx::pose_in_range(s, v2.data())) && (!ns || rtx::spheres_in_range(s, sph2.data()));
            CHECK(rtx::skinned_in_range(s, skin, m2) == fine);
            if (nc > 16) CHECK(!fine);                      // (bone 0 is followed by some corner of every such scene)
        }
    if (ns) {       // ... and of a radius factor
        for (float w : {nan, inf, -inf}) {
            std::vector<float> sc2(scale);
            sc2[0] = w;
            rtx::PoseMoves m2 = m;
            m2.radius_scale = sc2.data();
            rtx::skinned_prims(s, skin, m2, nullptr, sph2.data());
            CHECK(!rtx::spheres_in_range(s, sph2.data()) && !rtx::skinned_in_range(s, skin, m2));
        }
    }
    {   // a map that takes some of the scene beyond the bound and leaves the rest within: the two rules agree
        std::vector<float> mv2(moves);
        mv2[3] = 3.0f * s.scene_magnitude;
        rtx::PoseMoves m2 = m;
        m2.moves = mv2.data();
        rtx::skinned_prims(s, skin, m2, v2.data(), sph2.data());
        CHECK(rtx::skinned_in_range(s, skin, m2) == ((!nt || rtx::pose_in_range(s, v2.data())) && (!ns || rtx::spheres_in_range(s, sph2.data()))));
    }
}

static void run(const std::vector<float> &tris, const std::vector<float> &spheres, const std::vector<uint8_t> &kinds,
                const std::vector<float> &samples)
{
    RtxSceneDesc d;
    std::memset(&d, 0, sizeof d);
    d.width = d.height = 8;
    const float eye[3] = {0, 100, 200}, look[3] = {0, 0, -100000}, up[3] = {0, 1, 0};
    std::memcpy(d.eye, eye, 12);
    rtxh_camera_new(eye, look, up, d.u, d.v, d.w);
    d.distance = 288.0f;
    const float l[9] = {-10, 300, -10, 10, 300, -10, 0, 300, 0};
    std::memcpy(d.light_v0, l, 12); std::memcpy(d.light_v1, l + 3, 12); std::memcpy(d.light_v2, l + 6, 12);
    const size_t nt = tris.size() / 9, ns = spheres.size() / 4;
    d.n_tris = static_cast<uint32_t>(nt);
    d.n_spheres = static_cast<uint32_t>(ns);
    std::vector<float> rgb(3 * nt, 0.5f), srgb(3 * ns, 0.25f);
    d.v0v1v2 = tris.data(); d.rgb = rgb.data();
    d.spheres = spheres.data(); d.sphere_rgb = srgb.data();
    d.kinds = kinds.empty() ? nullptr : kinds.data();
    d.nb_ray = 1; d.nb_light_sample = 4;
    d.samples = samples.data(); d.n_samples = static_cast<uint32_t>(samples.size() / 2);
    d.reference_tree = RTX_REFTREE_NEVER;
    rtx::PreparedScene s;
    CHECK(rtx::prepare_scene(d, s) == RTX_OK);
    for (uint32_t n_moves : {1u, 2u, 7u, 300u}) through(s, n_moves);
}

int main()
{
    std::vector<float> samples(2 * 4096);
    for (size_t i = 0; i < samples.size(); ++i) samples[i] = float((i * 2654435761u) % 10007u) / 10007.0f;
    {   // no primitive at all: a PreparedScene as constructed
        rtx::PreparedScene none;
        for (uint32_t n_moves : {1u, 65536u}) through(none, n_moves);
    }
    for (uint32_t n : {13u, 255u, 256u, 257u})
        for (int arms = 0; arms < 3; ++arms) {      // both arms (every third a sphere), triangles alone, spheres alone
            std::vector<uint8_t> kinds(n);
            uint32_t nt = 0;
            for (uint32_t i = 0; i < n; ++i) nt += (kinds[i] = arms == 0 ? i % 3 == 2 : arms == 2) == 0;
            std::vector<float> tris(9 * static_cast<size_t>(nt)), spheres;
            if (nt) CHECK(rtxh_synthetic_mesh(12345ull, nt, tris.data()) == RTX_OK);
            for (uint32_t i = 0; i < n - nt; ++i) {
                const float sph[4] = {-80.0f + float(i % 17) * 8.0f, 40.0f + float(i % 13) * 10.0f, -50.0f + float(i % 11) * 9.0f,
                                      0.5f + 0.125f * float(i % 16)};
                spheres.insert(spheres.end(), sph, sph + 4);
            }
            run(tris, spheres, kinds, samples);
        }
    std::printf("skin sanitizer driver: %d failed checks\n", fails);
    return fails ? 1 : 0;
}
