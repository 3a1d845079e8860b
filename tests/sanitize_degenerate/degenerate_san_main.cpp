// Sanitizer leg for the host side over zero-area triangles (never on the GPU): scene_prep.cpp and host_helpers.cpp are
// compiled with -fsanitize=address,undefined together with this driver, which pushes the size scenes — an ordinary
// triangle and n point triangles at ONE point for n on both sides of the refit thresholds, nothing but segments on one
// line, nothing but points — and a 300-triangle thicket (a soup with every third triangle a point, an e1 = 0, an e2 = 0, a
// v1 = v2, an (a, a + e, a + 2e) or an (a, mid, b) triangle, a needle across the ground plane, a zero-radius sphere) through
// prepare_scene (tree builder, plane records, long-list prediction), both reference trees, and the four pose statements
// with each scene collapsed onto one point, folded and given back.  tests/test_degenerate_host.py builds and runs it;
// any report makes the process exit non-zero.
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
    uint32_t leaf_max = 0, width = 8, height = 8;
};

static bool same(const void *a, const void *b, size_t bytes) { return std::memcmp(a, b, bytes) == 0; }

static void check_streams(const rtx::PreparedScene &s, const std::vector<rtx::NodeRec> &nodes, const rtx::TriRec *tris, size_t n)
{
    // every record of the primitive array in exactly one leaf run, every box finite and around its run's boxes
    std::vector<int> seen(n, 0);
    for (const rtx::NodeRec &nd : nodes) {
        for (int k = 0; k < 3; ++k) CHECK(std::isfinite(nd.bmin[k]) && std::isfinite(nd.bmax[k]));
        if (!(nd.info & rtx::kLeafFlag)) continue;
        const size_t first = nd.info & rtx::kLeafIndexMask;
        CHECK(nd.link >= 1 && first + nd.link <= n);
        for (size_t j = first; j < first + nd.link && j < n; ++j) {
            ++seen[j];
            for (int k = 0; k < 3; ++k) CHECK(nd.bmin[k] <= tris[j].bmin[k] && nd.bmax[k] >= tris[j].bmax[k]);
        }
    }
    for (size_t j = 0; j < n; ++j) CHECK(seen[j] == 1);
    (void)s;
}

static void run(const Case &c, const std::vector<float> &samples)
{
    RtxSceneDesc d;
    std::memset(&d, 0, sizeof d);
    d.width = c.width; d.height = c.height;
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
    d.spheres = ns ? c.spheres.data() : nullptr; d.sphere_rgb = ns ? srgb.data() : nullptr;
    d.kinds = c.kinds.empty() ? nullptr : c.kinds.data();
    d.nb_ray = 1; d.nb_light_sample = 4;
    d.samples = samples.data(); d.n_samples = static_cast<uint32_t>(samples.size() / 2);
    d.accel = RTX_ACCEL_BVH; d.leaf_max = c.leaf_max; d.reference_tree = RTX_REFTREE_ALWAYS;
    rtx::PreparedScene s;
    CHECK(rtx::prepare_scene(d, s) == RTX_OK);
    const size_t n = s.tris.size(), ng = s.n_global;
    CHECK(n == nt + ns && s.ref_nodes.size() == 2 * n - 1);
    check_streams(s, s.nodes, s.tris.data(), n);
    CHECK(s.global_planes.size() == ng);
    for (const rtx::TriRec &g : s.global_planes) {
        CHECK(g.bmin[0] > 0.0f);                                 // finite or +infinity: never a NaN, never negative
        for (int k = 0; k < 3; ++k) CHECK(std::isfinite(g.e1[k]) && std::isfinite(g.e2[k]) && g.e2[k] > 0.0f);
    }
    // the long-list prediction over zero-volume boxes, once more per tile with a met array
    const uint32_t tiles_x = (c.width + 7u) / 8u, tiles_y = (c.height + 7u) / 8u;
    CHECK(s.long_tiles.size() == s.long_weights.size() && s.long_tiles.size() <= rtx::probe_long_cap(tiles_x * tiles_y));
    std::vector<uint8_t> met(s.nodes.size());
    for (uint32_t ty = 0; ty < tiles_y; ++ty)
        for (uint32_t tx = 0; tx < tiles_x; ++tx) {
            bool valid = false;
            rtx::probe_tile_weight(s, tx, ty, met.data(), &valid);
            CHECK(valid);
        }
    rtx::predict_long_tiles(s, 1u);
    CHECK(s.long_tiles.size() <= rtx::probe_long_cap(tiles_x * tiles_y));
    rtx::predict_long_tiles(s, rtx::kProbeLongWeight);

    rtx::PoseTables t;
    rtx::pose_tables(s, t);
    rtx::RebuildTables b;
    rtx::rebuild_tables(s, b);
    const size_t nn = b.nodes.size();
    // the poses: everything onto one point; every triangle folded (v1 := v2); every third triangle a point; back
    std::vector<std::vector<float>> poses(4, c.tris);
    for (size_t i = 0; i < nt; ++i) {
        for (int k = 0; k < 9; ++k) poses[0][9 * i + k] = float(3 + k % 3);
        std::memcpy(&poses[1][9 * i + 3], &poses[1][9 * i + 6], 12);
        if (i % 3 == 0) { std::memcpy(&poses[2][9 * i + 3], &poses[2][9 * i], 12); std::memcpy(&poses[2][9 * i + 6], &poses[2][9 * i], 12); }
    }
    std::vector<float> shrunk(c.spheres);
    for (size_t i = 0; i < ns; ++i) shrunk[4 * i + 3] = 0.0f;
    std::vector<rtx::TriRec> tris(n), sorted(n);
    std::vector<rtx::ShadeRec> shade(n), rshade(n);
    std::vector<rtx::NodeRec> nodes(s.nodes.size()), rnodes(nn);
    std::vector<uint64_t> keys(n - ng);
    std::vector<uint32_t> perm(n - ng);
    for (const std::vector<float> &pose : poses)
        for (int with_overlay = 0; with_overlay < 2; ++with_overlay) {
            rtx::PrimsOverlay ov;
            if (with_overlay && ns) ov.spheres = shrunk.data();
            if (with_overlay && nt) ov.rgb = rgb.data();
            CHECK(rtx::pose_in_range(s, pose.data()) && (!ns || rtx::spheres_in_range(s, shrunk.data())));
            rtx::posed_records(s, t, pose.data(), nullptr, tris.data(), shade.data(), nodes.data(), &ov);
            check_streams(s, nodes, tris.data(), n);
            for (size_t j = 0; j < n; ++j) CHECK(tris[j].idx == s.tris[j].idx);
            rtx::rebuilt_records(s, t, b, pose.data(), nullptr, keys.data(), perm.data(), sorted.data(), rshade.data(), rnodes.data(), &ov);
            check_streams(s, rnodes, sorted.data(), n);
            CHECK(same(shade.data(), rshade.data(), n * sizeof(rtx::ShadeRec)));
            std::vector<int> hit(n, 0);
            for (size_t p = 0; p + ng < n; ++p) {
                CHECK(perm[p] >= ng && perm[p] < n);
                if (perm[p] >= ng && perm[p] < n) { ++hit[perm[p]]; CHECK(same(&sorted[ng + p], &tris[perm[p]], sizeof(rtx::TriRec))); }
                if (p) CHECK(keys[p - 1] < keys[p] || (keys[p - 1] == keys[p] && perm[p - 1] < perm[p]));
            }
            for (size_t j = ng; j < n; ++j) CHECK(hit[j] == 1);
            // the plane records of the posed global triangles (rtx_scene_posed_pipeline_records' statement)
            for (size_t g = 0; g < ng; ++g) {
                rtx::TriRec plane;
                rtx::global_plane_statement(tris[g], &plane);
                CHECK(plane.bmin[0] > 0.0f && plane.idx == tris[g].idx);
            }
            std::vector<uint32_t> ref_rank;
            std::vector<rtx::NodeRec> stream;
            CHECK(rtx::posed_ref_tree(s, t, pose.data(), ref_rank, stream, &ov) == RTX_OK && stream.size() == 2 * n - 1 && ref_rank.size() == n);
            CHECK(rtx::rebuilt_ref_tree(s, t, pose.data(), perm.data(), ref_rank, stream, &ov) == RTX_OK && stream.size() == 2 * n - 1);
            size_t leaves = 0;
            for (const rtx::NodeRec &nd : stream)
                if (nd.info & rtx::kLeafFlag) { CHECK((nd.info & rtx::kLeafIndexMask) < n); ++leaves; }
            CHECK(leaves == n);
        }
}

int main()
{
    std::vector<float> samples(2 * 4096);
    rtxh_gen_samples(20261004ull, 4096, samples.data());
    const float one[9] = {0, 0, -5, 4, 0, -5, 0, 4, -6}, point[3] = {3, 4, -12};
    for (uint32_t n : {1u, 31u, 32u, 33u, 255u, 256u, 257u})
        for (uint32_t leaf_max : {0u, 1u}) {
            Case c;
            c.tris.assign(one, one + 9);
            for (uint32_t i = 0; i < 3 * n; ++i) c.tris.insert(c.tris.end(), point, point + 3);
            c.leaf_max = leaf_max;
            run(c, samples);
        }
    for (uint32_t leaf_max : {0u, 1u}) {
        Case seg, pts;
        for (int i = 0; i < 300; ++i)                          // (a, a + 7 e, a + 3 e) on one line: every sum exact
            for (int k : {0, 7, 3}) {
                const float v[3] = {-40.0f + 0.25f * float(i + k), 2.0f + 0.125f * float(i + k), -30.0f - 0.5f * float(i + k)};
                seg.tris.insert(seg.tris.end(), v, v + 3);
            }
        for (int i = 0; i < 252; ++i) {
            const float v[3] = {-9.0f + 3.0f * float(i % 7), 1.0f + 3.0f * float((i / 7) % 6), -30.0f + 3.0f * float(i / 42)};
            for (int k = 0; k < 3; ++k) pts.tris.insert(pts.tris.end(), v, v + 3);
        }
        seg.leaf_max = pts.leaf_max = leaf_max;
        run(seg, samples);
        run(pts, samples);
    }
    {
        Case c;                                                // the 300-triangle thicket
        c.tris.resize(9 * 300);
        CHECK(rtxh_synthetic_mesh(12345ull, 300, c.tris.data()) == RTX_OK);
        for (size_t i = 0; i < 300; i += 3) {
            float *v = &c.tris[9 * i];
            switch ((i / 3) % 6) {
            case 0: std::memcpy(v + 3, v, 12); std::memcpy(v + 6, v, 12); break;                       // a point
            case 1: std::memcpy(v + 3, v, 12); break;                                                  // e1 = 0
            case 2: std::memcpy(v + 6, v, 12); break;                                                  // e2 = 0
            case 3: std::memcpy(v + 3, v + 6, 12); break;                                              // v1 = v2
            case 4: for (int k = 0; k < 3; ++k) { v[k] = std::floor(v[k]); v[3 + k] = v[k] + float(5 + 2 * k); v[6 + k] = v[k] + 2.0f * float(5 + 2 * k); } break;
            default: for (int k = 0; k < 3; ++k) v[3 + k] = (v[k] + v[6 + k]) * 0.5f; break;           // (a, mid, b)
            }
        }
        const float needle[9] = {-9000, 0.5f, -9000, 0, 0.5f, 0, 9000, 0.5f, 9000};
        const float ground[9] = {-10000, 0, -10000, 10000, 0, -10000, 0, 0, 10000};
        std::memcpy(&c.tris[9 * 7], needle, 36);
        c.tris.insert(c.tris.end(), ground, ground + 9);
        c.spheres = {-40, 150, 30, 0, 105, 32, 20, 32};
        c.kinds.assign(303, 0);
        c.kinds[100] = c.kinds[200] = 1;
        c.width = 64; c.height = 48;
        run(c, samples);
        c.leaf_max = 1;
        run(c, samples);
    }
    std::printf("degenerate sanitizer driver: %d failed checks\n", fails);
    return fails ? 1 : 0;
}
