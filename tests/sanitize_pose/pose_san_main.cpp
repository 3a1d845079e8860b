// Sanitizer leg for the host statement of posing (never on the GPU): scene_prep.cpp and host_helpers.cpp are compiled with
// -fsanitize=address,undefined together with this driver, which pushes the small scenes of the pose tests — one triangle,
// two triangles around a sphere, soups of 255, 256 and 257 triangles with and without the ground, as a tree and as one
// leaf — through pose_tables, posed_records and posed_ref_tree.  tests/test_pose_host.py builds and runs it; any report
// makes the process exit non-zero.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../include/rtx.h"
#include "../../ray-tracer-rust_amd/csrc/scene_prep.h"

static int fails = 0;
#define CHECK(c) do { if (!(c)) { std::fprintf(stderr, "CHECK failed %s:%d: %s\n", __FILE__, __LINE__, #c); ++fails; } } while (0)

struct Case {
    std::vector<float> tris, spheres, pose;
    std::vector<uint8_t> kinds;
    uint32_t accel = RTX_ACCEL_BVH;
};

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
    d.n_tris = static_cast<uint32_t>(c.tris.size() / 9);
    std::vector<float> rgb(3 * static_cast<size_t>(d.n_tris), 0.5f), srgb(3 * (c.spheres.size() / 4), 0.25f);
    d.v0v1v2 = c.tris.data(); d.rgb = rgb.data();
    d.n_spheres = static_cast<uint32_t>(c.spheres.size() / 4);
    d.spheres = c.spheres.data(); d.sphere_rgb = srgb.data();
    d.kinds = c.kinds.empty() ? nullptr : c.kinds.data();
    d.nb_ray = 1; d.nb_light_sample = 4;
    d.samples = samples.data(); d.n_samples = static_cast<uint32_t>(samples.size() / 2);
    d.accel = c.accel; d.reference_tree = RTX_REFTREE_NEVER;
    rtx::PreparedScene s;
    CHECK(rtx::prepare_scene(d, s) == RTX_OK);
    rtx::PoseTables t;
    rtx::pose_tables(s, t);
    const size_t n = s.tris.size(), nn = s.nodes.size();
    CHECK(t.ranges.size() == 2 * nn && t.tri_of.size() == n && t.order.size() == nn && t.n_long <= nn);
    CHECK(t.ranges[0] == 0u && t.ranges[1] == n);                 // the root covers every record
    for (size_t i = 0; i < nn; ++i) {
        CHECK(t.ranges[2 * i + 1] >= 1u && t.ranges[2 * i] + t.ranges[2 * i + 1] <= n);
        const bool is_long = t.ranges[2 * t.order[i] + 1] > rtx::kPoseLaneMax;
        CHECK(is_long == (i < t.n_long));
    }
    // the identity pose gives the prepared records back
    std::vector<rtx::TriRec> tris(n);
    std::vector<rtx::ShadeRec> shade(n);
    std::vector<rtx::NodeRec> nodes(nn);
    CHECK(rtx::pose_in_range(s, c.tris.data()));
    rtx::posed_records(s, t, c.tris.data(), nullptr, tris.data(), shade.data(), nodes.data());
    CHECK(std::memcmp(tris.data(), s.tris.data(), n * sizeof(rtx::TriRec)) == 0);
    for (size_t i = 0; i < n; ++i) {
        CHECK(std::memcmp(shade[i].normal, s.shade[i].normal, 12) == 0 && shade[i].rank == i);
        CHECK(std::memcmp(shade[i].rgb, s.shade[i].rgb, 16) == 0);
    }
    for (size_t i = 0; i < nn; ++i)
        for (int k = 0; k < 3; ++k) {
            CHECK(nodes[i].bmin[k] == s.nodes[i].bmin[k] - s.cull_delta && nodes[i].bmax[k] == s.nodes[i].bmax[k] + s.cull_delta);
            CHECK(nodes[i].link == s.nodes[i].link && nodes[i].info == s.nodes[i].info);
        }
    // the pose, each output alone and all together, with ranks
    std::vector<uint32_t> rank(n);
    for (size_t i = 0; i < n; ++i) rank[i] = static_cast<uint32_t>(n - i);
    CHECK(rtx::pose_in_range(s, c.pose.data()));
    rtx::posed_records(s, t, c.pose.data(), rank.data(), tris.data(), shade.data(), nodes.data());
    std::vector<rtx::NodeRec> alone(nn);
    rtx::posed_records(s, t, c.pose.data(), nullptr, nullptr, nullptr, alone.data());
    CHECK(std::memcmp(alone.data(), nodes.data(), nn * sizeof(rtx::NodeRec)) == 0);
    rtx::posed_records(s, t, c.pose.data(), nullptr, nullptr, shade.data(), nullptr);
    rtx::posed_records(s, t, c.pose.data(), nullptr, nullptr, nullptr, nullptr);
    for (size_t j = 0; j < n; ++j)                                // every own box inside the root's
        for (int k = 0; k < 3; ++k) CHECK(tris[j].bmin[k] >= nodes[0].bmin[k] && tris[j].bmax[k] <= nodes[0].bmax[k]);
    std::vector<uint32_t> ref_rank;
    std::vector<rtx::NodeRec> stream;
    CHECK(rtx::posed_ref_tree(s, t, c.pose.data(), ref_rank, stream) == RTX_OK);
    CHECK(ref_rank.size() == n && stream.size() == 2 * n - 1);
    std::vector<float> bad = c.pose;
    if (!bad.empty()) {
        bad.back() = NAN;
        CHECK(!rtx::pose_in_range(s, bad.data()));
        bad.back() = s.scene_magnitude * 1.5f;
        CHECK(!rtx::pose_in_range(s, bad.data()));
    }
}

int main()
{
    std::vector<float> samples(2 * 4096);
    rtxh_gen_samples(20261004ull, 4096, samples.data());
    {
        Case c;
        c.tris = {0, 0, -5, 1, 0, -5, 0, 1, -5};
        c.pose = {0.5f, 0, -6, 2, 0.25f, -6, 0, 3, -7};
        run(c, samples);
    }
    {
        Case c;
        c.tris = {-3, 0, -8, -1, 0, -8, -2, 2, -8, 1, 0, -9, 3, 0, -9, 2, 2, -9};
        c.pose = {1.5f, 0.5f, -8.5f, 3.5f, 0.5f, -8.5f, 2.5f, 2.5f, -8.5f, -2.5f, 0.5f, -7.5f, -0.5f, 0.5f, -7.5f, -1.5f, 2.5f, -7.5f};
        c.spheres = {0, 1, -8, 1};
        c.kinds = {0, 1, 0};
        run(c, samples);
        c.accel = RTX_ACCEL_BRUTE;
        run(c, samples);
    }
    const float ground[9] = {-10000, 0, -10000, 10000, 0, -10000, 0, 0, 10000};
    for (uint32_t n : {255u, 256u, 257u})
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
    std::printf("pose sanitizer driver: %d failed checks\n", fails);
    return fails ? 1 : 0;
}
