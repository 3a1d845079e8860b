// Sanitizer leg for a scene whose sample table is replaced (never on the GPU): scene_prep.cpp and host_helpers.cpp are
// compiled with -fsanitize=address,undefined together with this driver, which takes small scenes — both arms, triangles
// alone, spheres alone, one primitive — through resample_scene with caller's tables allocated at their exact size (n = 1, 7,
// the created scene's count, one more pair than it), a table with entries that are not finite, refused calls, a reseed after
// a resample and back, and a seeded table of 2^31 pairs that no array holds.  After every accepted call the scene's derived
// arrays are compared with a scene CREATED with that table; after every refused one with what they were.  A read behind a
// table's end is a heap overflow the sanitizer reports.  tests/test_resample_host.py builds and runs it; any report makes
// the process exit non-zero.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "../../include/rtx.h"
#include "../../ray-tracer-rust_amd/csrc/scene_prep.h"

static int fails = 0;
#define CHECK(c) do { if (!(c)) { std::fprintf(stderr, "CHECK failed %s:%d: %s\n", __FILE__, __LINE__, #c); ++fails; } } while (0)

template <class T>
static bool same(const std::vector<T> &a, const std::vector<T> &b)
{
    return a.size() == b.size() && (a.empty() || std::memcmp(a.data(), b.data(), a.size() * sizeof(T)) == 0);
}

struct Inputs {
    std::vector<float> tris, spheres, rgb, srgb;
    std::vector<uint8_t> kinds;
    uint32_t nb_ray, nb_light;
};

static int create(const Inputs &in, const float *samples, uint32_t n, rtx::PreparedScene &s)
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
    d.n_tris = static_cast<uint32_t>(in.tris.size() / 9);
    d.n_spheres = static_cast<uint32_t>(in.spheres.size() / 4);
    d.v0v1v2 = in.tris.data(); d.rgb = in.rgb.data();
    d.spheres = in.spheres.data(); d.sphere_rgb = in.srgb.data();
    d.kinds = in.kinds.empty() ? nullptr : in.kinds.data();
    d.nb_ray = in.nb_ray; d.nb_light_sample = in.nb_light;
    d.samples = samples; d.n_samples = n;
    d.reference_tree = RTX_REFTREE_NEVER;
    return rtx::prepare_scene(d, s);
}

// everything a table decides, and what it must leave alone
static void same_derived(const rtx::PreparedScene &a, const rtx::PreparedScene &b, bool table_too)
{
    CHECK(same(a.light_points, b.light_points) && same(a.light_tour, b.light_tour) && same(a.light_order, b.light_order));
    CHECK(same(a.light_boxes, b.light_boxes) && std::memcmp(&a.shaft_delta, &b.shaft_delta, 4) == 0);
    CHECK(a.n_samples == b.n_samples);
    if (table_too) CHECK(same(a.samples, b.samples) && a.seeded == b.seeded && a.sample_seed == b.sample_seed);
    CHECK(a.nodes.size() == b.nodes.size() && a.tris.size() == b.tris.size() && std::memcmp(a.gamma_thr, b.gamma_thr, sizeof a.gamma_thr) == 0);
}

static void through(const Inputs &in, const std::vector<float> &first)
{
    const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
    const uint32_t n0 = static_cast<uint32_t>(first.size() / 2);
    rtx::PreparedScene s;
    CHECK(create(in, first.data(), n0, s) == RTX_OK);
    CHECK(!s.seeded && s.table_generation == 0);
    uint64_t generation = 0;
    for (uint32_t n : {1u, 7u, n0, n0 + 1u, 2u}) {
        // a caller's table of exactly n pairs on the heap, gone before the scene is read again
        rtx::PreparedScene want;
        {
            std::vector<float> t(2 * static_cast<size_t>(n));
            for (size_t i = 0; i < t.size(); ++i) t[i] = float((i * 40503u + n) % 9973u) / 9973.0f;
            CHECK(create(in, t.data(), n, want) == RTX_OK);
            CHECK(rtx::resample_scene(s, rtx::SampleSource{t.data(), 0, n}) == RTX_OK);
        }
        CHECK(s.table_generation == ++generation);
        same_derived(s, want, true);
        // refused: the scene stays
        rtx::PreparedScene before = s;
        CHECK(rtx::resample_scene(s, rtx::SampleSource{want.samples.data(), 0, 0}) == RTX_ERR_BAD_ARG);
        CHECK(rtx::resample_scene(s, rtx::SampleSource{nullptr, 5, 0}) == RTX_ERR_BAD_ARG);
        same_derived(s, before, true);
        CHECK(s.table_generation == generation);
        // entries that are not finite, at a light index and elsewhere: create's answer is the call's
        for (float bad : {nan, inf, -inf, 3e38f}) {
            std::vector<float> t(want.samples);
            t[0] = bad;
            t[t.size() - 1] = bad;
            rtx::PreparedScene made, kept = s;
            const int rc = create(in, t.data(), n, made);
            CHECK(rtx::resample_scene(s, rtx::SampleSource{t.data(), 0, n}) == rc);
            if (rc == RTX_OK) { same_derived(s, made, true); CHECK(s.table_generation == ++generation); }
            else { same_derived(s, kept, true); CHECK(s.table_generation == generation); }
        }
        // a reseed: the scene created with rtxh_gen_samples' table, and no array of the table's size
        for (uint64_t seed : {0ull, 1ull, ~0ull, 20261020ull}) {
            const uint32_t pairs = n + 3u * static_cast<uint32_t>(seed % 5u);
            std::vector<float> t(2 * static_cast<size_t>(pairs));
            rtxh_gen_samples(seed, pairs, t.data());
            rtx::PreparedScene made;
            CHECK(create(in, t.data(), pairs, made) == RTX_OK);
            CHECK(rtx::resample_scene(s, rtx::SampleSource{nullptr, seed, pairs}) == RTX_OK);
            CHECK(s.seeded && s.sample_seed == seed && s.samples.empty() && s.table_generation == ++generation);
            same_derived(s, made, false);
            const rtx::SampleSource src = rtx::sample_source(s);
            for (uint32_t k = 0; k < pairs; ++k) {
                float u, v;
                src.pair(k, &u, &v);
                CHECK(std::memcmp(&u, &t[2 * k], 4) == 0 && std::memcmp(&v, &t[2 * k + 1], 4) == 0);
            }
        }
        // ... and back to the caller's
        CHECK(rtx::resample_scene(s, rtx::SampleSource{want.samples.data(), 0, n}) == RTX_OK);
        ++generation;
        same_derived(s, want, true);
    }
    {   // 2^31 pairs and 2^32 - 1: the far end is computed
        for (uint32_t pairs : {0x80000000u, 0xFFFFFFFFu}) {
            CHECK(rtx::resample_scene(s, rtx::SampleSource{nullptr, 77, pairs}) == RTX_OK);
            CHECK(s.samples.empty() && s.n_samples == pairs);
            float u, v, w[2];
            rtx::sample_source(s).pair(static_cast<uint64_t>(pairs) - 1u, &u, &v);
            w[0] = rtx::sample_statement(77, 2ull * pairs - 2ull);
            w[1] = rtx::sample_statement(77, 2ull * pairs - 1ull);
            CHECK(u == w[0] && v == w[1] && u >= 0.0f && u < 1.0f && v >= 0.0f && v < 1.0f);
        }
    }
}

int main()
{
    std::vector<float> samples(2 * 61);
    for (size_t i = 0; i < samples.size(); ++i) samples[i] = float((i * 2654435761u) % 10007u) / 10007.0f;
    for (uint32_t n : {1u, 13u, 257u})
        for (int arms = 0; arms < 3; ++arms) {      // both arms (every third a sphere), triangles alone, spheres alone
            Inputs in;
            in.kinds.resize(n);
            uint32_t nt = 0;
            for (uint32_t i = 0; i < n; ++i) nt += (in.kinds[i] = arms == 0 ? i % 3 == 2 : arms == 2) == 0;
            in.tris.resize(9 * static_cast<size_t>(nt));
            if (nt) CHECK(rtxh_synthetic_mesh(12345ull, nt, in.tris.data()) == RTX_OK);
            for (uint32_t i = 0; i < n - nt; ++i) {
                const float sph[4] = {-80.0f + float(i % 17) * 8.0f, 40.0f + float(i % 13) * 10.0f, -50.0f + float(i % 11) * 9.0f,
                                      0.5f + 0.125f * float(i % 16)};
                in.spheres.insert(in.spheres.end(), sph, sph + 4);
            }
            in.rgb.assign(3 * static_cast<size_t>(nt), 0.5f);
            in.srgb.assign(3 * static_cast<size_t>(n - nt), 0.25f);
            for (uint32_t rays : {1u, 3u}) {
                in.nb_ray = rays;
                in.nb_light = rays == 1u ? 130u : 4u;           // two light batches, and one
                through(in, samples);
            }
        }
    std::printf("resample sanitizer driver: %d failed checks\n", fails);
    return fails ? 1 : 0;
}
