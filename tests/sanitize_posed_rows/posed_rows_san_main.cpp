// Sanitizer leg for the host statements behind rtx_render_view_rows_posed (never on the GPU): scene_prep.cpp and
// host_helpers.cpp are compiled with -fsanitize=address,undefined together with this driver, which pushes small scenes — a
// patch over a ground that the pose lifts, soups of 255 and 257 triangles with and without the ground, as a tree and as one
// leaf — through the plane statement (global_plane_statement over the posed records of the global triangles) and the posed
// aimed stream (stream_nearest_first over posed_records' node words), and the plane statement alone through the values
// where it could go wrong: zeros, subnormals, the largest finite edges, infinities and NaNs.
// tests/test_posed_rows_host.py builds and runs it; any report makes the process exit non-zero.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "../../include/rtx.h"
#include "../../ray-tracer-rust_amd/csrc/scene_prep.h"

static int fails = 0;
#define CHECK(c) do { if (!(c)) { std::fprintf(stderr, "CHECK failed %s:%d: %s\n", __FILE__, __LINE__, #c); ++fails; } } while (0)

static uint32_t bits_of(float x)
{
    uint32_t b;
    std::memcpy(&b, &x, 4);
    return b;
}

struct Case {
    std::vector<float> tris, pose;
    uint32_t accel = RTX_ACCEL_BVH;
    float eye[3] = {0, 100, 200};
};

static uint32_t tree_root(const rtx::PreparedScene &s) { return (s.n_global != 0u && s.nodes.size() > 2u) ? 2u : 0u; }

static void run(const Case &c, const std::vector<float> &samples)
{
    RtxSceneDesc d;
    std::memset(&d, 0, sizeof d);
    d.width = d.height = 8;
    const float look[3] = {0, 0, -100000}, up[3] = {0, 1, 0};
    std::memcpy(d.eye, c.eye, 12);
    rtxh_camera_new(c.eye, look, up, d.u, d.v, d.w);
    d.distance = 288.0f;
    const float l[9] = {-10, 300, -10, 10, 300, -10, 0, 300, 0};
    std::memcpy(d.light_v0, l, 12); std::memcpy(d.light_v1, l + 3, 12); std::memcpy(d.light_v2, l + 6, 12);
    d.n_tris = static_cast<uint32_t>(c.tris.size() / 9);
    std::vector<float> rgb(3 * static_cast<size_t>(d.n_tris), 0.5f);
    d.v0v1v2 = c.tris.data(); d.rgb = rgb.data();
    d.nb_ray = 1; d.nb_light_sample = 4;
    d.samples = samples.data(); d.n_samples = static_cast<uint32_t>(samples.size() / 2);
    d.accel = c.accel; d.reference_tree = RTX_REFTREE_NEVER;
    rtx::PreparedScene s;
    CHECK(rtx::prepare_scene(d, s) == RTX_OK);
    rtx::PoseTables t;
    rtx::pose_tables(s, t);
    const size_t n = s.tris.size(), nn = s.nodes.size();
    CHECK(s.global_planes.size() == s.n_global && s.n_global <= rtx::kMaxGlobalPrims);
    const float other_eye[3] = {-80, 150, -40};
    for (const std::vector<float> *pose : {&c.tris, &c.pose}) {
        std::vector<rtx::TriRec> tris(n);
        std::vector<rtx::NodeRec> nodes(nn);
        CHECK(rtx::pose_in_range(s, pose->data()));
        rtx::posed_records(s, t, pose->data(), nullptr, tris.data(), nullptr, nodes.data());
        // the planes: the identity pose gives the prepared scene's words
        std::vector<rtx::TriRec> planes(s.n_global);
        for (uint32_t i = 0; i < s.n_global; ++i) {
            rtx::global_plane_statement(tris[i], &planes[i]);
            CHECK(planes[i].idx == tris[i].idx && std::memcmp(planes[i].v0, tris[i].v0, 12) == 0);
            CHECK(planes[i].bmin[0] > 0.0f && planes[i].bmin[1] == 0.0f && planes[i].bmax[2] == 0.0f);
            for (int k = 0; k < 3; ++k) CHECK(planes[i].e2[k] > 0.0f);       // rounded UP from a sum of magnitudes
        }
        if (pose == &c.tris && s.n_global) CHECK(std::memcmp(planes.data(), s.global_planes.data(), s.n_global * sizeof(rtx::TriRec)) == 0);
        // the aimed stream over the posed node words: a pre-order of the same records
        for (const float *eye : {c.eye, other_eye}) {
            std::vector<rtx::NodeRec> aimed;
            if (s.primary_nodes.empty()) aimed = nodes;
            else rtx::stream_nearest_first(nodes, tree_root(s), eye, aimed);
            CHECK(aimed.size() == nn);
            size_t leaves_in = 0, leaves_out = 0;
            double sum_in = 0.0, sum_out = 0.0;
            for (size_t i = 0; i < nn && i < aimed.size(); ++i) {
                leaves_in += (nodes[i].info & rtx::kLeafFlag) != 0u;
                leaves_out += (aimed[i].info & rtx::kLeafFlag) != 0u;
                sum_in += static_cast<double>(nodes[i].bmin[0]) + nodes[i].bmax[1];
                sum_out += static_cast<double>(aimed[i].bmin[0]) + aimed[i].bmax[1];
                if (!(aimed[i].info & rtx::kLeafFlag) && i >= tree_root(s))
                    CHECK(aimed[i].info > i + 1 && aimed[i].info < aimed[i].link && aimed[i].link <= nn);
            }
            CHECK(leaves_in == leaves_out);
            CHECK(std::fabs(sum_in - sum_out) <= 1e-6 * (1.0 + std::fabs(sum_in)));
        }
    }
}

static void statement_at_the_edges()
{
    const float inf = std::numeric_limits<float>::infinity(), big = std::numeric_limits<float>::max();
    const float tiny = std::numeric_limits<float>::denorm_min();
    CHECK(bits_of(rtx::f32_successor(0.0f)) == 1u && rtx::f32_successor(1.0f) == std::nextafter(1.0f, inf));
    CHECK(rtx::f32_successor(big) == inf && rtx::f32_successor(inf) == inf && std::isnan(rtx::f32_successor(NAN)));
    CHECK(rtx::f32_successor(tiny) == std::nextafter(tiny, inf));
    const float edges[][6] = {
        {20000, 0, 0, 10000, 0, 20000},                 // main()'s ground: two W components of exactly 0
        {0, 0, 0, 0, 0, 0},                             // no area at all
        {tiny, 0, 0, 0, tiny, 0},                       // a product of 2^-298: exact in double, 0 in f32
        {big, big, big, -big, big, -big},               // W about 2^257: not "fine", K_d = inf
        {inf, 1, 1, 1, 1, 1},
        {NAN, 1, 1, 1, 2, 3},
        {1e30f, 1, 0, 0, 1e30f, 1},                     // W = 1e60 rounds to inf in f32
    };
    for (const auto &e : edges) {
        rtx::TriRec t{}, g;
        std::memset(&g, 0xAB, sizeof g);
        std::memcpy(t.e1, e, 12);
        std::memcpy(t.e2, e + 3, 12);
        t.v0[0] = 1.0f; t.v0[1] = -2.0f; t.v0[2] = 3.0f;
        t.idx = 77u;
        rtx::global_plane_statement(t, &g);
        CHECK(g.idx == 77u && g.v0[1] == -2.0f && g.bmin[1] == 0.0f && g.bmin[2] == 0.0f && g.bmax[0] == 0.0f);
        const bool finite = std::isfinite(e[0]) && std::fabs(e[0]) < 1e20f;
        CHECK(finite ? (std::isfinite(g.bmin[0]) && g.bmin[0] > 0.0f) : (g.bmin[0] == inf));
        for (int k = 0; k < 3; ++k) CHECK(std::isnan(g.e2[k]) || g.e2[k] > 0.0f);
    }
    rtx::TriRec ground{}, g;
    ground.e1[0] = 20000; ground.e2[0] = 10000; ground.e2[2] = 20000;
    rtx::global_plane_statement(ground, &g);
    CHECK(bits_of(g.e2[0]) == 1u && bits_of(g.e2[2]) == 1u && g.e1[1] == -4e8f && g.e2[1] == std::nextafter(4e8f, inf));
}

int main()
{
    std::vector<float> samples(2 * 4096);
    rtxh_gen_samples(20261004ull, 4096, samples.data());
    statement_at_the_edges();
    {   // a patch over a ground that the pose lifts
        Case c;
        c.tris = {-3, 2, -3, 3, 2, -3, 3, 2.5f, 3, -3, 2, -3, 3, 2.5f, 3, -3, 2.25f, 3, 1, 2.75f, 1, 2, 2.75f, 1, 1, 3, 2,
                  4, 0, -100, 4, 0, 100, -196, 0, 0};
        c.pose = c.tris;
        for (size_t k = c.pose.size() - 9 + 1; k < c.pose.size(); k += 3) c.pose[k] = 7.0f;
        c.eye[0] = 60; c.eye[1] = 40; c.eye[2] = 9;
        run(c, samples);
    }
    const float ground[9] = {-10000, 0, -10000, 10000, 0, -10000, 0, 0, 10000};
    for (uint32_t n : {255u, 257u})
        for (int with_ground = 0; with_ground < 2; ++with_ground)
            for (uint32_t accel : {static_cast<uint32_t>(RTX_ACCEL_BVH), static_cast<uint32_t>(RTX_ACCEL_BRUTE)}) {
                Case c;
                c.tris.resize(9 * static_cast<size_t>(n));
                c.pose.resize(9 * static_cast<size_t>(n));
                CHECK(rtxh_synthetic_mesh(12345ull, n, c.tris.data()) == RTX_OK);
                CHECK(rtxh_synthetic_mesh(777ull, n, c.pose.data()) == RTX_OK);
                if (with_ground) {
                    c.tris.insert(c.tris.end(), ground, ground + 9);
                    for (float g : ground) c.pose.push_back(0.5f * g);
                }
                c.accel = accel;
                run(c, samples);
            }
    std::printf("posed rows sanitizer driver: %d failed checks\n", fails);
    return fails ? 1 : 0;
}
