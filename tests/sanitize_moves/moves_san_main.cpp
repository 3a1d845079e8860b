// Sanitizer leg for the host statement of a moved pose (never on the GPU): scene_prep.cpp and host_helpers.cpp are compiled
// with -fsanitize=address,undefined together with this driver, which pushes small scenes — spheres alone, triangles alone,
// every third primitive a sphere at 255, 256 and 257 primitives — through moved_prims, move_groups_ok and the range rules
// with NaN and infinite moves, group values at, beyond and far beyond n_moves, RTX_MOVE_NONE, a NULL group array, and
// radius_scale NULL and given; a scene of no primitives at all (a PreparedScene as constructed) goes through the same.
// The moves and radius_scale arrays are allocated at their exact size, so an index that was not compared against n_moves
// is a heap overflow the sanitizer reports.  tests/test_moves_host.py builds and runs it; any report makes the process
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

// the statement once more, spelled out, for one point
static void point(const float *m, const float *p, float *out)
{
    for (int r = 0; r < 3; ++r) {
        const float a = m[4 * r] * p[0], b = m[4 * r + 1] * p[1], c = m[4 * r + 2] * p[2];
        const float ab = a + b, abc = ab + c;
        out[r] = abc + m[4 * r + 3];
    }
}

static void through(const rtx::PreparedScene &s, uint32_t n_moves)
{
    const size_t nt = s.rest_tri_vec.size(), ns = s.rest_sphere_vec.size(), n = s.n_tris;
    CHECK(nt + ns == n && s.rest_v0v1v2.size() == 9 * nt && s.rest_spheres.size() == 4 * ns);
    // exact-size arrays on the heap
    std::vector<float> moves(12 * static_cast<size_t>(n_moves)), scale(n_moves);
    for (uint32_t g = 0; g < n_moves; ++g) {
        std::memcpy(&moves[12 * static_cast<size_t>(g)], kIdentity, sizeof kIdentity);
        moves[12 * static_cast<size_t>(g) + 1] = 0.125f * float(g % 5);
        moves[12 * static_cast<size_t>(g) + 3] = 0.5f * float(g % 7) - 1.0f;
        moves[12 * static_cast<size_t>(g) + 11] = -0.25f * float(g % 3);
        scale[g] = 0.5f * float(g % 4);
    }
    std::vector<float> v(9 * nt), sph(4 * ns), v2(9 * nt), sph2(4 * ns);
    rtx::PoseMoves m;
    m.n_moves = n_moves;
    m.moves = moves.data();
    // NULL group: every primitive follows move 0; radius_scale NULL: radii copied
    CHECK(rtx::move_groups_ok(s, m));
    rtx::moved_prims(s, m, v.data(), sph.data());
    for (size_t t = 0; t < 3 * nt; ++t) {
        float want[3];
        point(moves.data(), &s.rest_v0v1v2[3 * t], want);
        CHECK(same(want, &v[3 * t], 12));
    }
    for (size_t i = 0; i < ns; ++i) CHECK(same(&sph[4 * i + 3], &s.rest_spheres[4 * i + 3], 4));
    rtx::moved_prims(s, m, nullptr, nullptr);      // either output may be NULL
    rtx::moved_prims(s, m, v2.data(), nullptr);
    rtx::moved_prims(s, m, nullptr, sph2.data());
    CHECK(same(v.data(), v2.data(), 4 * v.size()) && same(sph.data(), sph2.data(), 4 * sph.size()));
    // a group per Vec position: in range, RTX_MOVE_NONE, and the values the host check refuses
    std::vector<uint32_t> group(n);
    for (size_t i = 0; i < n; ++i) group[i] = i % 4 == 3 ? rtx::kMoveNone : static_cast<uint32_t>(i % n_moves);
    m.group = group.data();
    m.radius_scale = scale.data();
    CHECK(rtx::move_groups_ok(s, m));
    rtx::moved_prims(s, m, v.data(), sph.data());
    for (size_t t = 0; t < nt; ++t) {
        const uint32_t g = group[s.rest_tri_vec[t]];
        for (int k = 0; k < 3; ++k) {
            float want[3];
            if (g == rtx::kMoveNone) std::memcpy(want, &s.rest_v0v1v2[9 * t + 3 * k], 12);
            else point(&moves[12 * static_cast<size_t>(g)], &s.rest_v0v1v2[9 * t + 3 * k], want);
            CHECK(same(want, &v[9 * t + 3 * k], 12));
        }
    }
    for (size_t i = 0; i < ns; ++i) {
        const uint32_t g = group[s.rest_sphere_vec[i]];
        float want[4];
        std::memcpy(want, &s.rest_spheres[4 * i], 16);
        if (g != rtx::kMoveNone) {
            point(&moves[12 * static_cast<size_t>(g)], &s.rest_spheres[4 * i], want);
            want[3] = s.rest_spheres[4 * i + 3] * scale[g];
        }
        CHECK(same(want, &sph[4 * i], 16));
    }
    if (nt) CHECK(rtx::pose_in_range(s, v.data()));
    CHECK(rtx::moved_in_range(s, m));
    if (n) {
        const uint32_t bad[4] = {n_moves, n_moves + 1u, 0xFFFFFFFEu, 0x80000000u};
        for (uint32_t b : bad)
            for (size_t at : {size_t(0), n / 2, n - 1}) {
                std::vector<uint32_t> g2(group);
                g2[at] = b;
                m.group = g2.data();
                CHECK(!rtx::move_groups_ok(s, m));
                rtx::moved_prims(s, m, v2.data(), sph2.data());      // the statement takes it as RTX_MOVE_NONE
                g2[at] = rtx::kMoveNone;
                std::vector<float> v3(9 * nt), sph3(4 * ns);
                rtx::moved_prims(s, m, v3.data(), sph3.data());
                CHECK(same(v2.data(), v3.data(), 4 * v2.size()) && same(sph2.data(), sph3.data(), 4 * sph2.size()));
            }
        m.group = group.data();
    }
    // NaN and infinite entries of a move that is followed: the output leaves the range rule
    const float wild[3] = {std::numeric_limits<float>::quiet_NaN(), std::numeric_limits<float>::infinity(),
                           -std::numeric_limits<float>::infinity()};
    for (float w : wild)
        for (int at : {0, 3, 5, 10, 11}) {
            std::vector<float> mv2(moves);
            mv2[at] = w;
            rtx::PoseMoves m2 = m;
            m2.moves = mv2.data();
            m2.group = nullptr;
            rtx::moved_prims(s, m2, v2.data(), sph2.data());
            if (nt) CHECK(!rtx::pose_in_range(s, v2.data()));
            if (ns) CHECK(!rtx::spheres_in_range(s, sph2.data()));
            CHECK(rtx::moved_in_range(s, m2) == (nt + ns == 0));
        }
    if (ns) {       // ... and of a radius factor
        for (float w : wild) {
            std::vector<float> sc2(scale);
            sc2[0] = w;
            rtx::PoseMoves m2 = m;
            m2.radius_scale = sc2.data();
            m2.group = nullptr;
            rtx::moved_prims(s, m2, nullptr, sph2.data());
            CHECK(!rtx::spheres_in_range(s, sph2.data()) && !rtx::moved_in_range(s, m2));
        }
    }
    {   // a map that takes some of the scene beyond the bound and leaves the rest within: the two rules agree
        std::vector<float> mv2(moves);
        mv2[3] = 0.75f * s.scene_magnitude;
        rtx::PoseMoves m2 = m;
        m2.moves = mv2.data();
        rtx::moved_prims(s, m2, v2.data(), sph2.data());
        CHECK(rtx::moved_in_range(s, m2) == ((!nt || rtx::pose_in_range(s, v2.data())) && (!ns || rtx::spheres_in_range(s, sph2.data()))));
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
    // the rest geometry is the description's arrays, and the tables name each entry's Vec position
    CHECK(s.rest_v0v1v2 == tris && s.rest_spheres == spheres);
    size_t next_t = 0, next_s = 0;
    for (size_t i = 0; i < s.shade.size(); ++i) {
        if (s.shade[i].kind) CHECK(next_s < ns && s.rest_sphere_vec[next_s++] == i);
        else CHECK(next_t < nt && s.rest_tri_vec[next_t++] == i);
    }
    CHECK(next_t == nt && next_s == ns);
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
    std::printf("moves sanitizer driver: %d failed checks\n", fails);
    return fails ? 1 : 0;
}
