// Sanitizer leg for the host statement of a rebuilt pose (never on the GPU): scene_prep.cpp and host_helpers.cpp are
// compiled with -fsanitize=address,undefined together with this driver, which pushes small scenes — the ground alone, one
// to 33 triangles, two triangles around a sphere, spheres beside one triangle, coincident triangles, soups of 255, 256 and
// 257 triangles, each with and without the ground — through rebuild_tables, rebuilt_records (keys, sort, records, boxes) and
// rebuilt_ref_tree, and the key statement through NaNs, infinities and coordinates outside the frame.
// tests/test_rebuild_host.py builds and runs it; any report makes the process exit non-zero.
#include <algorithm>
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
    uint32_t accel = RTX_ACCEL_BVH, leaf_max = 0;
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
    d.accel = c.accel; d.leaf_max = c.leaf_max; d.reference_tree = RTX_REFTREE_NEVER;
    rtx::PreparedScene s;
    CHECK(rtx::prepare_scene(d, s) == RTX_OK);
    rtx::PoseTables t;
    rtx::pose_tables(s, t);
    rtx::RebuildTables b;
    rtx::rebuild_tables(s, b);
    const size_t n = s.tris.size(), ng = s.n_global, nt = n - ng, nn = b.nodes.size();
    const uint32_t leaf_max = c.leaf_max ? c.leaf_max : 4u;
    CHECK(s.leaf_max == leaf_max);
    CHECK(b.ranges.size() == 2 * nn && b.order.size() == nn && b.n_long <= nn && nn >= 1);
    CHECK(b.n_tree_tris + b.n_tree_spheres == nt);
    CHECK(b.ranges[0] == 0u && b.ranges[1] == n);                 // the root covers every record
    std::vector<uint32_t> covered(n, 0u);
    for (size_t i = 0; i < nn; ++i) {
        const uint32_t first = b.ranges[2 * i], count = b.ranges[2 * i + 1];
        CHECK(count >= 1u && first + count <= n);
        const bool is_long = b.ranges[2 * b.order[i] + 1] > rtx::kPoseLaneMax;
        CHECK(is_long == (i < b.n_long));
        const rtx::NodeRec &nd = b.nodes[i];
        if (nd.info & rtx::kLeafFlag) {
            CHECK((nd.info & rtx::kLeafIndexMask) == first && nd.link == count);
            CHECK(count <= leaf_max || (ng != 0 && first == 0u));
            for (uint32_t j = first; j < first + count; ++j) ++covered[j];
        } else {
            CHECK(nd.info > i + 1 && nd.info < nd.link && nd.link <= nn);
        }
    }
    for (size_t j = 0; j < n; ++j) CHECK(covered[j] == 1u);
    // the pose, each output alone and all together, with ranks
    std::vector<uint32_t> rank(n);
    for (size_t i = 0; i < n; ++i) rank[i] = static_cast<uint32_t>(n - i);
    std::vector<uint64_t> keys(nt);
    std::vector<uint32_t> perm(nt);
    std::vector<rtx::TriRec> tris(n), posed(n);
    std::vector<rtx::ShadeRec> shade(n);
    std::vector<rtx::NodeRec> nodes(nn), alone(nn);
    for (const std::vector<float> *pose : {&c.tris, &c.pose}) {
        rtx::rebuilt_records(s, t, b, pose->data(), rank.data(), keys.data(), perm.data(), tris.data(), shade.data(), nodes.data());
        rtx::rebuilt_records(s, t, b, pose->data(), nullptr, nullptr, nullptr, nullptr, nullptr, alone.data());
        CHECK(std::memcmp(alone.data(), nodes.data(), nn * sizeof(rtx::NodeRec)) == 0);
        rtx::rebuilt_records(s, t, b, pose->data(), nullptr, keys.data(), nullptr, nullptr, nullptr, nullptr);
        rtx::rebuilt_records(s, t, b, pose->data(), nullptr, nullptr, nullptr, nullptr, nullptr, nullptr);
        rtx::posed_records(s, t, pose->data(), rank.data(), posed.data(), nullptr, nullptr);
        std::vector<uint32_t> seen(perm);
        std::sort(seen.begin(), seen.end());
        for (size_t p = 0; p < nt; ++p) {
            CHECK(seen[p] == ng + p);
            CHECK(std::memcmp(&tris[ng + p], &posed[perm[p]], sizeof(rtx::TriRec)) == 0);
            if (p) CHECK(keys[p - 1] < keys[p] || (keys[p - 1] == keys[p] && perm[p - 1] < perm[p]));
            const bool sphere = s.shade[tris[ng + p].idx].kind != 0u;
            CHECK((keys[p] >> 63) == (sphere ? 1u : 0u));
            CHECK(sphere == (p >= b.n_tree_tris));
        }
        for (size_t j = 0; j < n; ++j)                                // every own box inside the root's
            for (int k = 0; k < 3; ++k) CHECK(tris[j].bmin[k] >= nodes[0].bmin[k] && tris[j].bmax[k] <= nodes[0].bmax[k]);
        std::vector<uint32_t> ref_rank;
        std::vector<rtx::NodeRec> stream;
        CHECK(rtx::rebuilt_ref_tree(s, t, pose->data(), perm.data(), ref_rank, stream) == RTX_OK);
        CHECK(ref_rank.size() == n && stream.size() == 2 * n - 1);
        for (const rtx::NodeRec &nd : stream)
            if (nd.info & rtx::kLeafFlag) CHECK((nd.info & rtx::kLeafIndexMask) < n);
    }
}

static void keys_at_the_edges()
{
    const float inf = INFINITY, m = 10000.0f, s = rtx::rebuild_key_scale(m);
    const float lo[3] = {-m, -m, -m}, hi[3] = {m, m, m}, nan3[3] = {NAN, NAN, NAN}, out[3] = {3e38f, 3e38f, 3e38f};
    const float pinf[3] = {inf, inf, inf}, ninf[3] = {-inf, -inf, -inf}, below[3] = {-3e38f, -2.0f * m, -m - 1.0f};
    const uint64_t all = (1ull << 63) - 1u;
    CHECK(rtx::rebuild_key_statement(lo, lo, false, m, s) == 0u);
    CHECK(rtx::rebuild_key_statement(hi, hi, false, m, s) == all);
    CHECK(rtx::rebuild_key_statement(hi, hi, true, m, s) == ((1ull << 63) | all));
    CHECK(rtx::rebuild_key_statement(nan3, nan3, false, m, s) == 0u);
    CHECK(rtx::rebuild_key_statement(ninf, pinf, false, m, s) == 0u);          // (-inf + inf: a NaN)
    CHECK(rtx::rebuild_key_statement(out, out, false, m, s) == all);           // (the sum overflows to +inf: the last cell)
    CHECK(rtx::rebuild_key_statement(pinf, pinf, false, m, s) == all);
    CHECK(rtx::rebuild_key_statement(ninf, ninf, false, m, s) == 0u);
    CHECK(rtx::rebuild_key_statement(below, below, true, m, s) == 1ull << 63);
    const float zero[3] = {0, 0, 0};
    CHECK(rtx::rebuild_key_statement(zero, zero, false, m, s) == (7ull << 60));   // cell 2^20 on every axis
    const float s0 = rtx::rebuild_key_scale(0.0f);                                  // a scene at the origin: S = +inf
    CHECK(rtx::rebuild_key_statement(zero, zero, false, 0.0f, s0) == 0u);           // (0 * inf: a NaN)
}

int main()
{
    std::vector<float> samples(2 * 4096);
    rtxh_gen_samples(20261004ull, 4096, samples.data());
    keys_at_the_edges();
    const float ground[9] = {-10000, 0, -10000, 10000, 0, -10000, 0, 0, 10000};
    {
        Case c;
        c.tris.assign(ground, ground + 9);
        for (float g : ground) c.pose.push_back(0.5f * g);
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
        c.accel = RTX_ACCEL_BVH;
        for (int i = 0; i < 10; ++i) {               // eleven spheres: the sphere run splits
            const float sph[4] = {float(3 * i) - 15.0f, 2.0f, -20.0f + float(i % 3), 0.5f + 0.25f * float(i)};
            c.spheres.insert(c.spheres.end(), sph, sph + 4);
            c.kinds.push_back(1);
        }
        run(c, samples);
    }
    for (uint32_t n : {1u, 2u, 4u, 5u, 9u, 20u, 32u, 33u, 255u, 256u, 257u})
        for (int with_ground = 0; with_ground < 2; ++with_ground)
            for (uint32_t leaf_max : {0u, 1u, 7u}) {
                Case c;
                c.tris.resize(9 * static_cast<size_t>(n));
                c.pose.resize(9 * static_cast<size_t>(n));
                CHECK(rtxh_synthetic_mesh(12345ull, n, c.tris.data()) == RTX_OK);
                CHECK(rtxh_synthetic_mesh(777ull, n, c.pose.data()) == RTX_OK);
                if (n == 20u) {                      // coincident triangles: equal keys
                    for (int i = 4; i < 9; ++i) std::memcpy(&c.tris[9 * i], &c.tris[27], 36);
                    for (int i = 2; i < 10; ++i) std::memcpy(&c.pose[9 * i], &c.pose[9 * 12], 36);
                }
                if (with_ground) {
                    c.tris.insert(c.tris.end(), ground, ground + 9);
                    for (float g : ground) c.pose.push_back(0.5f * g);
                }
                c.leaf_max = leaf_max;
                run(c, samples);
            }
    std::printf("rebuild sanitizer driver: %d failed checks\n", fails);
    return fails ? 1 : 0;
}
