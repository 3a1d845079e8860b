// Sanitizer leg for the mean of N frames (never on the GPU): host_helpers.cpp and scene_prep.cpp are compiled with
// -fsanitize=address,undefined together with this driver, which runs the two host statements over n = 0, 1, 3, 4, 5 and 257
// records held in heap blocks of their exact size — the inputs at an address that is not a multiple of 4, out_rgb at every
// byte offset 0 .. 3 — with records that hold -0.0, denormals, 2^61, infinities and NaN, `first` over a block of 0xAA bytes,
// hit counts that pass 255 and 2^32, every frame count the call accepts at its ends, and every refused call.  Each result
// is compared with the statement applied record by record.  A read or write behind a block's end is a heap overflow the
// sanitizer reports.  tests/test_accum_host.py builds and runs it; any report makes the process exit non-zero.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "../../include/rtx.h"
#include "../../ray-tracer-rust_amd/csrc/scene_prep.h"

static int fails = 0;
#define CHECK(c) do { if (!(c)) { std::fprintf(stderr, "CHECK failed %s:%d: %s\n", __FILE__, __LINE__, #c); ++fails; } } while (0)

static uint64_t state = 20261021ull;
static uint32_t draw()
{
    state += 0x9E3779B97F4A7C15ull;
    uint64_t z = state;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return static_cast<uint32_t>((z ^ (z >> 31)) >> 32);
}

static float value()
{
    const float inf = std::numeric_limits<float>::infinity();
    const float special[] = {-0.0f, 0.0f, 1e-45f, 1e-40f, 0x1p61f, -0x1p61f, 0x1p-61f, inf, -inf, std::numeric_limits<float>::quiet_NaN(),
                             1.0f, 0.5f, 3.0e38f};
    const uint32_t r = draw();
    if (r % 3u == 0u) return special[(r >> 8) % (sizeof special / sizeof special[0])];
    return static_cast<float>(r >> 8) * 0x1p-24f;
}

static RtxPixelShade record()
{
    RtxPixelShade s;
    for (float &x : s.linear) x = value();
    for (uint8_t &b : s.rgb8) b = static_cast<uint8_t>(draw());
    const uint8_t hits[] = {0, 1, 255, 2};
    s.hits = hits[draw() % 4u];
    return s;
}

static bool same_bytes(const void *a, const void *b, size_t n) { return n == 0 || std::memcmp(a, b, n) == 0; }

static void through(const float *thr, uint32_t n, size_t rgb_offset)
{
    const uint32_t frames = 4;
    std::vector<std::vector<RtxPixelShade>> in(frames, std::vector<RtxPixelShade>(n));
    for (auto &f : in)
        for (RtxPixelShade &s : f) s = record();
    // the accumulator by the library, in a block of its exact size, one byte off every alignment
    std::vector<char> block(static_cast<size_t>(n) * sizeof(RtxAccumPixel) + 1, static_cast<char>(0xAA));
    RtxAccumPixel *acc = reinterpret_cast<RtxAccumPixel *>(block.data() + 1);
    std::vector<RtxAccumPixel> want(n);
    for (uint32_t k = 0; k < frames; ++k) {
        std::vector<char> shade_block(static_cast<size_t>(n) * sizeof(RtxPixelShade) + 1);
        if (n) std::memcpy(shade_block.data() + 1, in[k].data(), static_cast<size_t>(n) * sizeof(RtxPixelShade));
        CHECK(rtxh_accum_add(n, reinterpret_cast<const RtxPixelShade *>(shade_block.data() + 1), acc, k == 0 ? 1u : 0u) == RTX_OK);
        for (uint32_t i = 0; i < n; ++i) rtx::accum_add_statement(k == 0, in[k][i], &want[i]);
        CHECK(same_bytes(acc, want.data(), static_cast<size_t>(n) * sizeof(RtxAccumPixel)));
    }
    const uint32_t counts[] = {frames, 1u, 3u, 7u, RTX_MAX_MEAN_FRAMES};
    for (uint32_t n_frames : counts) {
        std::vector<uint8_t> rgb_block(static_cast<size_t>(n) * 3u + rgb_offset, 0xAA);
        std::vector<char> out_block(static_cast<size_t>(n) * sizeof(RtxPixelShade) + 1, static_cast<char>(0xAA));
        uint8_t *rgb = rgb_block.data() + rgb_offset;
        RtxPixelShade *out = reinterpret_cast<RtxPixelShade *>(out_block.data() + 1);
        uint8_t spare = 0xAA;
        if (rgb_block.empty()) rgb = &spare;
        CHECK(rtxh_accum_resolve(thr, n, acc, n_frames, rgb, out) == RTX_OK);
        for (uint32_t i = 0; i < n; ++i) {
            const RtxPixelShade s = rtx::accum_resolve_statement(thr, n_frames, want[i]);
            CHECK(same_bytes(&s, reinterpret_cast<const char *>(out) + i * sizeof s, sizeof s) && same_bytes(s.rgb8, rgb + 3u * i, 3));
        }
        for (size_t b = 0; b < rgb_offset; ++b) CHECK(rgb_block[b] == 0xAA);
        // each output alone
        std::vector<uint8_t> rgb_only(static_cast<size_t>(n) * 3u + rgb_offset, 0xAA);
        uint8_t none = 0xAA;                                      // (an empty block has no address: n == 0 at offset 0)
        CHECK(rtxh_accum_resolve(thr, n, acc, n_frames, rgb_only.empty() ? &none : rgb_only.data() + rgb_offset, nullptr) == RTX_OK);
        CHECK(none == 0xAA);
        CHECK(same_bytes(rgb_only.data(), rgb_block.data(), rgb_only.size()));
        std::vector<char> out_only(out_block.size(), static_cast<char>(0xAA));
        CHECK(rtxh_accum_resolve(thr, n, acc, n_frames, nullptr, reinterpret_cast<RtxPixelShade *>(out_only.data() + 1)) == RTX_OK);
        CHECK(same_bytes(out_only.data(), out_block.data(), out_only.size()));
    }
}

int main()
{
    float thr[256];
    CHECK(rtx::build_gamma_thresholds(thr) == RTX_OK);
    const uint32_t sizes[] = {0u, 1u, 3u, 4u, 5u, 257u};
    for (uint32_t n : sizes)
        for (size_t offset = 0; offset < 4; ++offset) through(thr, n, offset);

    // the colour rule and the saturation
    const float inf = std::numeric_limits<float>::infinity();
    RtxAccumPixel a = {{std::numeric_limits<float>::quiet_NaN(), -inf, -1.0f}, 256u};
    RtxPixelShade s = rtx::accum_resolve_statement(thr, 1u, a);
    CHECK(s.rgb8[0] == 0 && s.rgb8[1] == 255 && s.rgb8[2] == 0 && s.hits == 255);
    a = RtxAccumPixel{{inf, 0.0f, 3.0f}, 254u};
    s = rtx::accum_resolve_statement(thr, 3u, a);
    CHECK(s.rgb8[0] == 255 && s.rgb8[1] == 0 && s.rgb8[2] == 255 && s.hits == 254 && s.linear[2] == 1.0f);
    a = RtxAccumPixel{{0.0f, 0.0f, 0.0f}, 0xFFFFFFFFu};
    RtxPixelShade hit = {{0.0f, 0.0f, 0.0f}, {0, 0, 0}, 255};
    rtx::accum_add_statement(false, hit, &a);
    CHECK(a.hit_frames == 0u);                                   // a plain u32 addition

    // refused calls: nothing is read or written
    RtxAccumPixel one = {{1.0f, 2.0f, 3.0f}, 1u};
    RtxPixelShade out;
    uint8_t rgb[3];
    CHECK(rtxh_accum_add(1, nullptr, &one, 0) == RTX_ERR_BAD_ARG && rtxh_accum_add(1, &hit, nullptr, 0) == RTX_ERR_BAD_ARG);
    CHECK(rtxh_accum_add(0, nullptr, nullptr, 1) == RTX_ERR_BAD_ARG && rtxh_accum_add(0, &hit, &one, 1) == RTX_OK);
    CHECK(one.hit_frames == 1u && one.sum[0] == 1.0f);
    CHECK(rtxh_accum_resolve(nullptr, 1, &one, 1, rgb, &out) == RTX_ERR_BAD_ARG);
    CHECK(rtxh_accum_resolve(thr, 1, nullptr, 1, rgb, &out) == RTX_ERR_BAD_ARG);
    CHECK(rtxh_accum_resolve(thr, 1, &one, 1, nullptr, nullptr) == RTX_ERR_BAD_ARG);
    CHECK(rtxh_accum_resolve(thr, 1, &one, 0, rgb, &out) == RTX_ERR_BAD_ARG);
    CHECK(rtxh_accum_resolve(thr, 1, &one, RTX_MAX_MEAN_FRAMES + 1u, rgb, &out) == RTX_ERR_BAD_ARG);
    CHECK(rtxh_accum_resolve(thr, 0, &one, 0, rgb, &out) == RTX_ERR_BAD_ARG && rtxh_accum_resolve(thr, 0, &one, 1, rgb, &out) == RTX_OK);
    CHECK(rtxh_accum_resolve(thr, 1, &one, RTX_MAX_MEAN_FRAMES, rgb, &out) == RTX_OK && out.linear[0] == 0x1p-16f && out.hits == 1);

    std::printf("accum sanitizer driver: %d failed checks\n", fails);
    return fails ? 1 : 0;
}
