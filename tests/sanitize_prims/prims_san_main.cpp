// Sanitizer leg for the host statement of a pose that states every field of a primitive (never on the GPU):
// scene_prep.cpp and host_helpers.cpp are compiled with -fsanitize=address,undefined together with this driver, which
// pushes small scenes — spheres alone, spheres between triangles, every third primitive a sphere at 255, 256 and 257
// primitives, each with and without the ground — through overlay_records, posed_records, rebuilt_records and both
// reference trees with every combination of the three optional arrays, and sphere_statement and spheres_in_range through
// NaNs, infinities, a zero and a negative radius and boxes at and beyond the bound.
// tests/test_prims_host.py builds and runs it; any report makes the process exit non-zero.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../include/rtx.h"
#include "../../ray-tracer-rust_amd/csrc/scene_prep.h"

static int fails = 0;
#define CHECK(c) do { if (!(c)) { std::fprintf(stderr, "CHECK failed %s:%d: %s\n", __FILE__, __LINE__, #c); ++fails; } } while (0)

struct Case {
    std::vector<float> tris, spheres;
    std::vector<uint8_t> kinds;
    uint32_t accel = RTX_ACCEL_BVH, leaf_max = 0;
};

static bool same(const void *a, const void *b, size_t bytes) { return std::memcmp(a, b, bytes) == 0; }

static void run(const Case &c, const std::vector<float> &samples)
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
    const size_t nt = c.tris.size() / 9, ns = c.spheres.size() / 4;
    d.n_tris = static_cast<uint32_t>(nt);
    d.n_spheres = static_cast<uint32_t>(ns);
    std::vector<float> rgb(3 * nt, 0.5f), srgb(3 * ns, 0.25f);
    d.v0v1v2 = c.tris.data(); d.rgb = rgb.data();
    d.spheres = c.spheres.data(); d.sphere_rgb = srgb.data();
    d.kinds = c.kinds.empty() ? nullptr : c.kinds.data();
    d.nb_ray = 1; d.nb_light_sample = 4;
    d.samples = samples.data(); d.n_samples = static_cast<uint32_t>(samples.size() / 2);
    d.accel = c.accel; d.leaf_max = c.leaf_max; d.reference_tree = RTX_REFTREE_NEVER;
    rtx::PreparedScene s;
    CHECK(rtx::prepare_scene(d, s) == RTX_OK);
    rtx::PoseTables t;
    rtx::pose_tables(s, t);
    rtx::RebuildTables b;
    rtx::rebuild_tables(s, b);
    const size_t n = s.tris.size(), ng = s.n_global, nn = b.nodes.size();
    CHECK(n == nt + ns && t.sphere_of.size() == n && t.tri_of.size() == n);
    size_t next_t = 0, next_s = 0;
    for (size_t i = 0; i < n; ++i) {
        if (s.shade[i].kind) CHECK(t.sphere_of[i] == next_s++ && t.tri_of[i] == rtx::kPoseNoTriangle);
        else CHECK(t.tri_of[i] == next_t++ && t.sphere_of[i] == rtx::kPoseNoTriangle);
    }
    // the pose: every sphere elsewhere with another radius, every colour another
    std::vector<float> pose(c.tris), moved(c.spheres), prgb(3 * nt), psrgb(3 * ns);
    for (size_t i = 0; i < pose.size(); ++i) pose[i] = 0.75f * pose[i] + float(i % 5);
    for (size_t i = 0; i < ns; ++i) {
        moved[4 * i] += 7.0f; moved[4 * i + 1] -= 3.0f; moved[4 * i + 2] *= 0.5f;
        moved[4 * i + 3] = i % 3 == 0 ? 0.0f : 0.5f * float(i % 7);
    }
    for (size_t i = 0; i < prgb.size(); ++i) prgb[i] = float(i % 11) / 11.0f;
    for (size_t i = 0; i < psrgb.size(); ++i) psrgb[i] = float(i % 13) / 13.0f;
    CHECK(rtx::spheres_in_range(s, c.spheres.data()) && rtx::spheres_in_range(s, moved.data()));
    // the identity overlay: the uploaded words
    std::vector<rtx::TriRec> ot(n), tris(n), plain(n);
    std::vector<rtx::ShadeRec> os(n), shade(n), pshade(n);
    rtx::PrimsOverlay ident;
    ident.spheres = c.spheres.data(); ident.rgb = rgb.data(); ident.sphere_rgb = srgb.data();
    if (!ns) ident.spheres = ident.sphere_rgb = nullptr;
    if (!nt) ident.rgb = nullptr;
    rtx::overlay_records(s, t, ident, ot.data(), os.data());
    CHECK(same(ot.data(), s.tris.data(), n * sizeof(rtx::TriRec)) && same(os.data(), s.shade.data(), n * sizeof(rtx::ShadeRec)));
    std::vector<rtx::NodeRec> nodes(s.nodes.size()), pnodes(s.nodes.size()), rnodes(nn), rpnodes(nn);
    std::vector<uint64_t> keys(n - ng), pkeys(n - ng);
    std::vector<uint32_t> perm(n - ng), pperm(n - ng);
    rtx::posed_records(s, t, pose.data(), nullptr, plain.data(), pshade.data(), pnodes.data());
    rtx::posed_records(s, t, pose.data(), nullptr, tris.data(), shade.data(), nodes.data(), &ident);
    CHECK(same(tris.data(), plain.data(), n * sizeof(rtx::TriRec)) && same(shade.data(), pshade.data(), n * sizeof(rtx::ShadeRec)));
    CHECK(same(nodes.data(), pnodes.data(), nodes.size() * sizeof(rtx::NodeRec)));
    for (unsigned mask = 0; mask < 8u; ++mask) {
        rtx::PrimsOverlay ov;
        if ((mask & 1u) && ns) ov.spheres = moved.data();
        if ((mask & 2u) && nt) ov.rgb = prgb.data();
        if ((mask & 4u) && ns) ov.sphere_rgb = psrgb.data();
        const float *v = nt ? pose.data() : nullptr;                   // (no triangles: no vertex array)
        rtx::overlay_records(s, t, ov, ot.data(), nullptr);
        rtx::overlay_records(s, t, ov, nullptr, os.data());
        rtx::posed_records(s, t, v, nullptr, tris.data(), shade.data(), nodes.data(), &ov);
        rtx::posed_records(s, t, v, nullptr, nullptr, nullptr, nullptr, &ov);
        for (size_t j = 0; j < n; ++j) {
            const uint32_t idx = tris[j].idx;
            CHECK(idx == s.tris[j].idx);
            const rtx::ShadeRec &sh = shade[idx];
            if (sh.kind) {
                const float *p = (ov.spheres ? moved.data() : c.spheres.data()) + 4 * t.sphere_of[idx];
                CHECK(same(tris[j].v0, p, 12) && same(sh.normal, p, 12) && tris[j].e1[1] == p[3] && tris[j].e1[0] == p[3] * p[3]);
                for (int k = 0; k < 3; ++k) CHECK(tris[j].bmin[k] == p[k] - p[3] && tris[j].bmax[k] == p[k] + p[3]);
                CHECK(same(sh.rgb, (ov.sphere_rgb ? psrgb.data() : srgb.data()) + 3 * t.sphere_of[idx], 12));
            } else {
                CHECK(same(tris[j].v0, pose.data() + 9 * t.tri_of[idx], 12));
                CHECK(same(sh.rgb, (ov.rgb ? prgb.data() : rgb.data()) + 3 * t.tri_of[idx], 12));
            }
            for (int k = 0; k < 3; ++k) CHECK(tris[j].bmin[k] >= nodes[0].bmin[k] && tris[j].bmax[k] <= nodes[0].bmax[k]);
        }
        rtx::rebuilt_records(s, t, b, v, nullptr, keys.data(), perm.data(), plain.data(), pshade.data(), rnodes.data(), &ov);
        rtx::rebuilt_records(s, t, b, v, nullptr, nullptr, nullptr, nullptr, nullptr, rpnodes.data(), &ov);
        CHECK(same(rnodes.data(), rpnodes.data(), nn * sizeof(rtx::NodeRec)));
        CHECK(same(pshade.data(), shade.data(), n * sizeof(rtx::ShadeRec)));
        for (size_t p = 0; p + ng < n; ++p) {
            CHECK(perm[p] >= ng && perm[p] < n && same(&plain[ng + p], &tris[perm[p]], sizeof(rtx::TriRec)));
            if (p) CHECK(keys[p - 1] < keys[p] || (keys[p - 1] == keys[p] && perm[p - 1] < perm[p]));
        }
        std::vector<uint32_t> ref_rank;
        std::vector<rtx::NodeRec> stream;
        CHECK(rtx::posed_ref_tree(s, t, v, ref_rank, stream, &ov) == RTX_OK && stream.size() == 2 * n - 1);
        CHECK(rtx::rebuilt_ref_tree(s, t, v, perm.data(), ref_rank, stream, &ov) == RTX_OK && ref_rank.size() == n);
        for (const rtx::NodeRec &nd : stream)
            if (nd.info & rtx::kLeafFlag) CHECK((nd.info & rtx::kLeafIndexMask) < n);
    }
}

static void statement_and_range()
{
    float v0[3], e1[3] = {9, 9, 9}, lo[3], hi[3], origin[3];
    const float a[4] = {1.5f, -2.25f, 1e-3f, 0.1f};
    rtx::sphere_statement(a, v0, e1, lo, hi, origin);
    CHECK(same(v0, a, 12) && same(origin, a, 12) && e1[0] == 0.1f * 0.1f && e1[1] == 0.1f && e1[2] == 9.0f);
    for (int k = 0; k < 3; ++k) CHECK(lo[k] == a[k] - 0.1f && hi[k] == a[k] + 0.1f);
    const float neg[4] = {0, 0, 0, -2.0f};                      // a negative radius: the words Sphere::new makes of it
    rtx::sphere_statement(neg, v0, e1, lo, hi, origin);
    CHECK(e1[0] == 4.0f && e1[1] == -2.0f && lo[0] == 2.0f && hi[0] == -2.0f);
    rtx::PreparedScene s;
    s.n_spheres = 1;
    s.scene_magnitude = 100.0f;
    const float inside[4] = {90, -90, 0, 10}, at[4] = {0, 0, 0, 100}, over[4] = {90.0f, 0, 0, 10.00001f}, big[4] = {0, 0, 0, 3e38f};
    const float nan4[4] = {0, NAN, 0, 1}, inf4[4] = {0, 0, INFINITY, 1}, rinf[4] = {0, 0, 0, INFINITY}, rnan[4] = {0, 0, 0, NAN};
    CHECK(rtx::spheres_in_range(s, inside) && rtx::spheres_in_range(s, at) && rtx::spheres_in_range(s, neg));
    CHECK(!rtx::spheres_in_range(s, over) && !rtx::spheres_in_range(s, big));
    CHECK(!rtx::spheres_in_range(s, nan4) && !rtx::spheres_in_range(s, inf4) && !rtx::spheres_in_range(s, rinf) && !rtx::spheres_in_range(s, rnan));
    s.n_spheres = 0;
    CHECK(rtx::spheres_in_range(s, nullptr));
}

int main()
{
    std::vector<float> samples(2 * 4096);
    rtxh_gen_samples(20261004ull, 4096, samples.data());
    statement_and_range();
    const float ground[9] = {-10000, 0, -10000, 10000, 0, -10000, 0, 0, 10000};
    {
        Case c;                                       // two triangles around a sphere
        c.tris = {-3, 0, -8, -1, 0, -8, -2, 2, -8, 1, 0, -9, 3, 0, -9, 2, 2, -9};
        c.spheres = {0, 1, -8, 1};
        c.kinds = {0, 1, 0};
        run(c, samples);
        c.accel = RTX_ACCEL_BRUTE;
        run(c, samples);
    }
    for (uint32_t n : {1u, 4u, 5u, 13u, 33u})         // spheres alone
        for (uint32_t leaf_max : {0u, 1u}) {
            Case c;
            for (uint32_t i = 0; i < n; ++i) {
                const float sph[4] = {float(3 * i) - 15.0f, 2.0f + float(i % 4), -20.0f + float(i % 3), 0.5f + 0.25f * float(i % 9)};
                c.spheres.insert(c.spheres.end(), sph, sph + 4);
            }
            c.leaf_max = leaf_max;
            run(c, samples);
        }
    for (uint32_t n : {3u, 255u, 256u, 257u})         // every third primitive a sphere
        for (int with_ground = 0; with_ground < 2; ++with_ground) {
            Case c;
            c.kinds.resize(n);
            uint32_t nt = 0;
            for (uint32_t i = 0; i < n; ++i) nt += (c.kinds[i] = i % 3 == 2) == 0;
            c.tris.resize(9 * static_cast<size_t>(nt));
            CHECK(rtxh_synthetic_mesh(12345ull, nt, c.tris.data()) == RTX_OK);
            for (uint32_t i = 0; i < n - nt; ++i) {
                const float sph[4] = {-80.0f + float(i % 17) * 8.0f, 40.0f + float(i % 13) * 10.0f, -50.0f + float(i % 11) * 9.0f,
                                      0.5f + 0.125f * float(i % 16)};
                c.spheres.insert(c.spheres.end(), sph, sph + 4);
            }
            if (with_ground) {
                c.tris.insert(c.tris.end(), ground, ground + 9);
                c.kinds.insert(c.kinds.begin() + 1, 0);
            }
            run(c, samples);
        }
    std::printf("prims sanitizer driver: %d failed checks\n", fails);
    return fails ? 1 : 0;
}
