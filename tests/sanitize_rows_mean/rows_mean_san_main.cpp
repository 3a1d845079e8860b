// Sanitizer leg for a frame of the mean through the render pipeline (never on the GPU): scene_prep.cpp and host_helpers.cpp
// are compiled with -fsanitize=address,undefined together with this driver, which runs light_walk_statement over seeded
// tables — seeds 0, 1, 2^64 - 1 and 20261020; 7, 129 and 4,099 pairs; counts 0, 1, 7, 128, 129 and 257; one and two rays per
// pixel; the scene's own triangle and another — with every output in a heap block of its exact size (and each output alone,
// the others NULL), and compares each with what resample_scene leaves in a twin scene reseeded with the same (seed, n_pairs);
// a light whose points overflow.
// A read or write behind a block's end is a heap overflow the sanitizer reports.  tests/test_rows_mean_host.py builds and runs
// it; any report makes the process exit non-zero.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>

#include "../../include/rtx.h"
#include "../../ray-tracer-rust_amd/csrc/scene_prep.h"

static int fails = 0;
#define CHECK(c) do { if (!(c)) { std::fprintf(stderr, "CHECK failed %s:%d: %s\n", __FILE__, __LINE__, #c); ++fails; } } while (0)

static const float kTris[3 * 9] = {-50.0f, 0.0f, -50.0f, 50.0f, 0.0f, -50.0f, 0.0f, 0.0f, 60.0f,
                                   -5.0f, 1.0f, -5.0f, 5.0f, 1.0f, -5.0f, 0.0f, 9.0f, 0.0f,
                                   2.0f, 3.0f, 4.0f, 6.0f, 3.0f, 4.0f, 4.0f, 7.0f, 5.0f};
static const float kRgb[3 * 3] = {0.5f, 0.5f, 0.5f, 0.9f, 0.2f, 0.1f, 0.1f, 0.3f, 0.8f};
static const float kOwnLight[9] = {-3.0f, 40.0f, -3.0f, 3.0f, 40.0f, -3.0f, 0.0f, 40.0f, 3.0f};
static const float kOtherLight[9] = {20.0f, 15.0f, 1.0f, 22.0f, 15.0f, 1.0f, 21.0f, 18.0f, 2.0f};

static int make_scene(uint32_t nb_ray, uint32_t count, const float light[9], const std::vector<float> &table, rtx::PreparedScene &out)
{
    RtxSceneDesc d;
    std::memset(&d, 0, sizeof d);
    d.width = 16; d.height = 12;
    const float eye[3] = {0.0f, 12.0f, 40.0f}, u[3] = {1.0f, 0.0f, 0.0f}, v[3] = {0.0f, -1.0f, 0.0f}, w[3] = {0.0f, 0.0f, 1.0f};
    std::memcpy(d.eye, eye, 12); std::memcpy(d.u, u, 12); std::memcpy(d.v, v, 12); std::memcpy(d.w, w, 12);
    d.distance = 20.0f;
    std::memcpy(d.light_v0, light, 12); std::memcpy(d.light_v1, light + 3, 12); std::memcpy(d.light_v2, light + 6, 12);
    d.n_tris = 3; d.v0v1v2 = kTris; d.rgb = kRgb;
    d.nb_ray = nb_ray; d.nb_light_sample = count;
    d.samples = table.data(); d.n_samples = static_cast<uint32_t>(table.size() / 2);
    return rtx::prepare_scene(d, out);
}

template <class T>
static std::unique_ptr<T[]> exact(size_t n) { return std::unique_ptr<T[]>(new T[n]); }      // (n == 0: a block of no bytes)

static void one(uint32_t nb_ray, uint32_t count, const float light[9], uint64_t seed, uint32_t n_pairs)
{
    std::vector<float> table(2 * 64);
    for (size_t i = 0; i < table.size(); ++i) table[i] = static_cast<float>((i * 37u) % 101u) / 101.0f;
    rtx::PreparedScene scene, twin;
    CHECK(make_scene(nb_ray, count, light, table, scene) == RTX_OK);
    CHECK(make_scene(nb_ray, count, light, table, twin) == RTX_OK);
    CHECK(rtx::resample_scene(twin, rtx::SampleSource{nullptr, seed, n_pairs}) == RTX_OK);
    const size_t n = static_cast<size_t>(nb_ray) * count;
    const rtx::SampleSource src{nullptr, seed, n_pairs};
    auto order = exact<uint32_t>(n);
    auto boxes = exact<float>(6u * nb_ray);
    auto delta = exact<float>(1);
    rtx::light_walk_statement(scene, light, count, src, order.get(), boxes.get(), delta.get());
    CHECK(twin.light_order.size() == n && (n == 0 || std::memcmp(order.get(), twin.light_order.data(), n * 4u) == 0));
    CHECK(twin.light_boxes.size() == 6u * nb_ray && std::memcmp(boxes.get(), twin.light_boxes.data(), 24u * nb_ray) == 0);
    CHECK(std::memcmp(delta.get(), &twin.shaft_delta, 4) == 0 && std::isfinite(delta[0]));
    // each output alone
    auto order2 = exact<uint32_t>(n);
    rtx::light_walk_statement(scene, light, count, src, order2.get(), nullptr, nullptr);
    CHECK(n == 0 || std::memcmp(order2.get(), order.get(), n * 4u) == 0);
    auto boxes2 = exact<float>(6u * nb_ray);
    rtx::light_walk_statement(scene, light, count, src, nullptr, boxes2.get(), nullptr);
    CHECK(std::memcmp(boxes2.get(), boxes.get(), 24u * nb_ray) == 0);
    auto delta2 = exact<float>(1);
    rtx::light_walk_statement(scene, light, count, src, nullptr, nullptr, delta2.get());
    CHECK(std::memcmp(delta2.get(), delta.get(), 4) == 0);
    // the scene the statement was asked about is as it was created
    CHECK(!scene.seeded && scene.n_samples == 64u && scene.table_generation == 0u);
}

int main()
{
    const uint64_t seeds[] = {0ull, 1ull, ~0ull, 20261020ull};
    const uint32_t pairs[] = {7u, 129u, 4099u};
    const uint32_t counts[] = {0u, 1u, 7u, 128u, 129u, 257u};
    int runs = 0;
    for (uint32_t nb_ray = 1; nb_ray <= 2; ++nb_ray)
        for (uint32_t count : counts)
            for (const float *light : {kOwnLight, kOtherLight})
                for (uint64_t seed : seeds)
                    for (uint32_t n_pairs : pairs) {
                        one(nb_ray, count, light, seed, n_pairs);
                        ++runs;
                    }
    // a light whose points overflow: the bounds that are not finite do not count (shaft_delta_of), the margin stays a number —
    // over a scene that was created it always is: magnitude * 2^-16 cannot overflow
    {
        const float far_light[9] = {3e38f, 3e38f, 3e38f, -3e38f, 3e38f, -3e38f, 3e38f, -3e38f, 3e38f};
        std::vector<float> table(2 * 64, 0.25f);
        rtx::PreparedScene scene;
        CHECK(make_scene(1, 7, kOwnLight, table, scene) == RTX_OK);
        auto delta = exact<float>(1);
        auto boxes = exact<float>(6);
        rtx::light_walk_statement(scene, far_light, 7, rtx::SampleSource{nullptr, 5ull, 4099u}, nullptr, boxes.get(), delta.get());
        CHECK(std::isfinite(delta[0]) && delta[0] >= scene.shaft_delta);
    }
    std::printf("rows mean sanitizer driver: %d walks, %d failed checks\n", runs, fails);
    return fails ? 1 : 0;
}
