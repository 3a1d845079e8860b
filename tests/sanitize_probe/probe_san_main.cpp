// Sanitizer leg for the host statement of the long primary walks (never on the GPU): scene_prep.cpp and host_helpers.cpp
// are compiled with -fsanitize=address,undefined together with this driver, which prepares both meshes of models/ (the
// ground last, as main() does) at several frame sizes — the prediction runs inside prepare_scene — and walks every tile
// once more through probe_tile_weight with a met array.  tests/test_probe_prediction_host.py builds and runs it; any
// report makes the process exit non-zero.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/rtx.h"
#include "../../ray-tracer-rust_amd/csrc/scene_prep.h"

static int fails = 0;
#define CHECK(c) do { if (!(c)) { std::fprintf(stderr, "CHECK failed %s:%d: %s\n", __FILE__, __LINE__, #c); ++fails; } } while (0)

static void run(const std::vector<float> &mesh, uint32_t width, uint32_t height, const std::vector<float> &samples, bool expect_some,
                bool mesh_in_view)
{
    std::vector<float> tris(mesh);
    const float ground[9] = {-10000, 0, -10000, 10000, 0, -10000, 0, 0, 10000};
    tris.insert(tris.end(), ground, ground + 9);
    RtxSceneDesc d;
    std::memset(&d, 0, sizeof d);
    d.width = width;
    d.height = height;
    const float eye[3] = {0, 100, 200}, look[3] = {0, 0, -100000}, up[3] = {0, 1, 0};
    std::memcpy(d.eye, eye, 12);
    rtxh_camera_new(eye, look, up, d.u, d.v, d.w);
    d.distance = 288.0f;
    const float l[9] = {-10, 300, -10, 10, 300, -10, 0, 300, 0};
    std::memcpy(d.light_v0, l, 12); std::memcpy(d.light_v1, l + 3, 12); std::memcpy(d.light_v2, l + 6, 12);
    d.n_tris = static_cast<uint32_t>(tris.size() / 9);
    std::vector<float> rgb(3 * static_cast<size_t>(d.n_tris), 0.5f);
    d.v0v1v2 = tris.data(); d.rgb = rgb.data();
    d.nb_ray = 2; d.nb_light_sample = 4;
    d.samples = samples.data(); d.n_samples = static_cast<uint32_t>(samples.size() / 2);
    d.accel = RTX_ACCEL_BVH; d.reference_tree = RTX_REFTREE_NEVER;
    rtx::PreparedScene s;
    CHECK(rtx::prepare_scene(d, s) == RTX_OK);
    const uint32_t tiles_x = (width + 7u) / 8u, tiles_y = (height + 7u) / 8u, n_tiles = tiles_x * tiles_y;
    CHECK(s.long_tiles.size() == s.long_weights.size() && s.long_tiles.size() <= rtx::probe_long_cap(n_tiles));
    CHECK(s.long_tiles.empty() ? s.long_bits.empty() : s.long_bits.size() == (n_tiles + 31u) / 32u);
    if (expect_some) CHECK(s.long_tiles.size() >= rtx::kProbeLongMinTiles);
    else CHECK(s.long_tiles.empty() || s.long_tiles.size() >= rtx::kProbeLongMinTiles);
    uint32_t bits = 0;
    for (uint32_t w : s.long_bits) bits += static_cast<uint32_t>(__builtin_popcount(w));
    CHECK(bits == s.long_tiles.size());
    for (size_t i = 0; i < s.long_tiles.size(); ++i) {
        CHECK(s.long_tiles[i] < n_tiles && s.long_weights[i] >= rtx::kProbeLongWeight);
        CHECK((s.long_bits[s.long_tiles[i] >> 5] >> (s.long_tiles[i] & 31u)) & 1u);
        if (i) CHECK(s.long_weights[i] <= s.long_weights[i - 1]);
    }
    std::vector<uint8_t> met(s.nodes.size());
    size_t listed = 0, heavy = 0;
    for (uint32_t ty = 0; ty < tiles_y; ++ty)
        for (uint32_t tx = 0; tx < tiles_x; ++tx) {
            std::fill(met.begin(), met.end(), 0);
            bool valid = false;
            const uint32_t w = rtx::probe_tile_weight(s, tx, ty, met.data(), &valid);
            CHECK(valid);
            const uint32_t t = ty * tiles_x + tx;
            const bool bit = !s.long_bits.empty() && ((s.long_bits[t >> 5] >> (t & 31u)) & 1u);
            if (bit) { CHECK(w >= rtx::kProbeLongWeight); ++listed; }
            if (w >= rtx::kProbeLongWeight && !s.long_tiles.empty() && s.long_tiles.size() < rtx::probe_long_cap(n_tiles)) CHECK(bit);
            if (w >= rtx::kProbeLongWeight) ++heavy;
        }
    CHECK(listed == s.long_tiles.size());
    if (s.long_tiles.empty()) CHECK(heavy < rtx::kProbeLongMinTiles || rtx::probe_long_cap(n_tiles) < rtx::kProbeLongMinTiles);
    // another threshold, the lists made anew: everything with a weight, then nothing
    rtx::predict_long_tiles(s, 1u);
    CHECK(s.long_tiles.size() <= rtx::probe_long_cap(n_tiles) && (n_tiles < 256u || !mesh_in_view || !s.long_tiles.empty()));
    rtx::predict_long_tiles(s, 0xFFFFFFFFu);
    CHECK(s.long_tiles.empty() && s.long_bits.empty());
}

int main(int argc, char **argv)
{
    const std::string models = argc > 1 ? argv[1] : "../../models";
    std::vector<float> samples(2 * 4096);
    rtxh_gen_samples(20261004ull, 4096, samples.data());
    for (const char *name : {"big_bunny.obj", "bunny.obj"}) {
        float *t = nullptr;
        const int n = rtxh_import_obj((models + "/" + name).c_str(), &t);
        CHECK(n > 0);
        if (n <= 0) continue;
        const std::vector<float> mesh(t, t + 9 * static_cast<size_t>(n));
        rtxh_free(t);
        const bool small = std::strcmp(name, "bunny.obj") == 0;
        run(mesh, 256, 256, samples, false, !small);       // (the centre crop of the frame holds the big mesh only)
        run(mesh, 203, 117, samples, false, !small);
        run(mesh, 1920, 1080, samples, !small, !small);  // the big mesh's silhouette; the small mesh lies in a few tiles: dropped
        run(mesh, 8, 8, samples, false, false);
    }
    if (fails) { std::fprintf(stderr, "probe_san: %d failed checks\n", fails); return 1; }
    std::printf("probe_san: OK\n");
    return 0;
}
