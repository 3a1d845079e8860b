// Sanitizer leg for the adaptive mean of N frames (never on the GPU): host_helpers.cpp and scene_prep.cpp are compiled
// with -fsanitize=address,undefined together with this driver, which runs the two host statements over rectangles of
// 1 x 1, 8 x 8, 9 x 8, 19 x 13 and 37 x 27 pixels held in heap blocks of their exact size — the arrays at an address that is
// not a multiple of 4, out_rgb at every byte offset 0 .. 3 — with records that hold -0.0, denormals, 2^61, infinities and
// NaN, `first` over blocks of 0xAA bytes, with and without tile states, under rules that stop tiles at once, late and
// never, and every refused call.  Each result is compared with the statements applied pixel by pixel, tile by tile.  A read
// or write behind a block's end is a heap overflow the sanitizer reports.  tests/test_adapt_host.py builds and runs it; any
// report makes the process exit non-zero.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "../../include/rtx.h"
#include "../../ray-tracer-rust_amd/csrc/scene_prep.h"

static int fails = 0;
#define CHECK(c) do { if (!(c)) { std::fprintf(stderr, "CHECK failed %s:%d: %s\n", __FILE__, __LINE__, #c); ++fails; } } while (0)

static uint64_t state = 20261022ull;
static uint32_t draw()
{
    state += 0x9E3779B97F4A7C15ull;
    uint64_t z = state;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return static_cast<uint32_t>((z ^ (z >> 31)) >> 32);
}

static float value(bool tame)
{
    const float inf = std::numeric_limits<float>::infinity();
    const float special[] = {-0.0f, 0.0f, 1e-45f, 1e-40f, 0x1p61f, -0x1p61f, 0x1p-61f, inf, -inf, std::numeric_limits<float>::quiet_NaN(),
                             1.0f, 0.5f, 3.0e38f};
    const uint32_t r = draw();
    if (!tame && r % 3u == 0u) return special[(r >> 8) % (sizeof special / sizeof special[0])];
    return static_cast<float>(r >> 8) * 0x1p-24f;
}

static RtxPixelShade record(bool tame)
{
    RtxPixelShade s;
    for (float &x : s.linear) x = value(tame);
    for (uint8_t &b : s.rgb8) b = static_cast<uint8_t>(draw());
    const uint8_t hits[] = {0, 1, 255, 2};
    s.hits = hits[draw() % 4u];
    return s;
}

static bool same_bytes(const void *a, const void *b, size_t n) { return n == 0 || std::memcmp(a, b, n) == 0; }

// a rectangle through `frames` adds and a resolve; tame: colours in [0, 1) only (tiles stop at different frames)
static void through(const float *thr, uint32_t nx, uint32_t ny, bool with_tiles, const RtxAdaptRule &rule, bool tame, size_t rgb_offset)
{
    const uint32_t frames = 5, n = nx * ny, tiles_x = (nx + 7u) / 8u, tiles_y = (ny + 7u) / 8u, n_tiles = tiles_x * tiles_y;
    std::vector<char> block(static_cast<size_t>(n) * sizeof(RtxMomentPixel) + 1, static_cast<char>(0xAA));
    std::vector<char> tile_block(static_cast<size_t>(n_tiles) * sizeof(RtxTileState) + 1, static_cast<char>(0xAA));
    RtxMomentPixel *mom = reinterpret_cast<RtxMomentPixel *>(block.data() + 1);
    RtxTileState *tiles = with_tiles ? reinterpret_cast<RtxTileState *>(tile_block.data() + 1) : nullptr;
    std::vector<RtxMomentPixel> want(n);
    std::vector<RtxTileState> want_tiles(n_tiles);
    uint32_t skipped = 0;
    for (uint32_t k = 0; k < frames; ++k) {
        std::vector<RtxPixelShade> in(n);
        for (RtxPixelShade &s : in) s = record(tame);
        std::vector<char> shade_block(static_cast<size_t>(n) * sizeof(RtxPixelShade) + 1);
        std::memcpy(shade_block.data() + 1, in.data(), static_cast<size_t>(n) * sizeof(RtxPixelShade));
        CHECK(rtxh_moment_add(nx, ny, reinterpret_cast<const RtxPixelShade *>(shade_block.data() + 1), mom, tiles, k == 0 ? 1u : 0u,
                              with_tiles ? &rule : nullptr) == RTX_OK);
        for (uint32_t t = 0; t < n_tiles; ++t) {
            if (with_tiles && k != 0 && rtx::tile_stopped(rule, want_tiles[t])) { ++skipped; continue; }
            float err = 0.0f;
            const uint32_t x0 = (t % tiles_x) * 8u, y0 = (t / tiles_x) * 8u;
            for (uint32_t y = y0; y < y0 + 8u && y < ny; ++y)
                for (uint32_t x = x0; x < x0 + 8u && x < nx; ++x) {
                    rtx::moment_add_statement(k == 0, in[y * nx + x], &want[y * nx + x]);
                    const float e = rtx::moment_error_statement(want[y * nx + x]);
                    CHECK(e >= 0.0f);                                   // never NaN, never negative
                    err = err < e ? e : err;
                }
            want_tiles[t].frames = k == 0 ? 1u : want_tiles[t].frames + 1u;
            want_tiles[t].err = err;
        }
        CHECK(same_bytes(mom, want.data(), static_cast<size_t>(n) * sizeof(RtxMomentPixel)));
        if (with_tiles) CHECK(same_bytes(tiles, want_tiles.data(), static_cast<size_t>(n_tiles) * sizeof(RtxTileState)));
        else CHECK(tile_block[1] == static_cast<char>(0xAA));
    }
    if (with_tiles && rule.min_frames <= 2u && rule.max_variance == std::numeric_limits<float>::infinity()) CHECK(skipped == n_tiles * (frames - 2u));
    CHECK(block[0] == static_cast<char>(0xAA) && tile_block[0] == static_cast<char>(0xAA));
    std::vector<uint8_t> rgb_block(static_cast<size_t>(n) * 3u + rgb_offset, 0xAA);
    std::vector<char> out_block(static_cast<size_t>(n) * sizeof(RtxPixelShade) + 1, static_cast<char>(0xAA));
    uint8_t *rgb = rgb_block.data() + rgb_offset;
    RtxPixelShade *out = reinterpret_cast<RtxPixelShade *>(out_block.data() + 1);
    CHECK(rtxh_moment_resolve(thr, n, mom, rgb, out) == RTX_OK);
    for (uint32_t i = 0; i < n; ++i) {
        const RtxPixelShade s = rtx::moment_resolve_statement(thr, want[i]);
        CHECK(same_bytes(&s, reinterpret_cast<const char *>(out) + i * sizeof s, sizeof s) && same_bytes(s.rgb8, rgb + 3u * i, 3));
    }
    for (size_t b = 0; b < rgb_offset; ++b) CHECK(rgb_block[b] == 0xAA);
    std::vector<uint8_t> rgb_only(rgb_block.size(), 0xAA);
    CHECK(rtxh_moment_resolve(thr, n, mom, rgb_only.data() + rgb_offset, nullptr) == RTX_OK);
    CHECK(same_bytes(rgb_only.data(), rgb_block.data(), rgb_only.size()));
    std::vector<char> out_only(out_block.size(), static_cast<char>(0xAA));
    CHECK(rtxh_moment_resolve(thr, n, mom, nullptr, reinterpret_cast<RtxPixelShade *>(out_only.data() + 1)) == RTX_OK);
    CHECK(same_bytes(out_only.data(), out_block.data(), out_only.size()));
}

int main()
{
    float thr[256];
    CHECK(rtx::build_gamma_thresholds(thr) == RTX_OK);
    const float inf = std::numeric_limits<float>::infinity();
    const uint32_t shapes[][2] = {{1u, 1u}, {8u, 8u}, {9u, 8u}, {19u, 13u}, {37u, 27u}};
    const RtxAdaptRule rules[] = {{5u, 0.0f}, {2u, inf}, {1u, 0.0f}, {2u, 0.03f}, {3u, 0.02f}};
    size_t offset = 0;
    for (const auto &shape : shapes)
        for (const RtxAdaptRule &rule : rules)
            for (int tame = 0; tame < 2; ++tame) {
                through(thr, shape[0], shape[1], true, rule, tame != 0, offset++ % 4u);
                through(thr, shape[0], shape[1], false, rule, tame != 0, offset++ % 4u);
            }

    // the statements' corners: one frame has variance exactly 0; a NaN and inf - inf count as 0; the own count divides
    RtxPixelShade s = {{0.3f, 0.7f, 0.1f}, {0, 0, 0}, 3};
    RtxMomentPixel m;
    std::memset(&m, 0xAA, sizeof m);
    rtx::moment_add_statement(true, s, &m);
    CHECK(m.frames == 1u && m.hit_frames == 1u && m.sumsq[1] == 0.7f * 0.7f && rtx::moment_error_statement(m) == 0.0f);
    CHECK(rtx::tile_stopped(RtxAdaptRule{1u, 0.0f}, RtxTileState{1u, 0.0f}) && !rtx::tile_stopped(RtxAdaptRule{2u, inf}, RtxTileState{1u, 0.0f}));
    CHECK(!rtx::tile_stopped(RtxAdaptRule{1u, 1.0f}, RtxTileState{9u, std::numeric_limits<float>::quiet_NaN()}));
    RtxPixelShade wild = {{inf, std::numeric_limits<float>::quiet_NaN(), 3.0e38f}, {0, 0, 0}, 0};
    rtx::moment_add_statement(false, wild, &m);
    CHECK(m.frames == 2u && m.hit_frames == 1u && rtx::moment_error_statement(m) == 0.0f);
    m = RtxMomentPixel{{3.0f, 0.0f, 1.0f}, 300u, {9.0f, 0.0f, 1.0f}, 3u};
    const RtxPixelShade r = rtx::moment_resolve_statement(thr, m);
    CHECK(r.linear[0] == 1.0f && r.linear[2] == 1.0f / 3.0f && r.hits == 255 && r.rgb8[0] == 255 && r.rgb8[1] == 0);

    // refused calls: nothing is read or written
    RtxMomentPixel one = {{1.0f, 2.0f, 3.0f}, 1u, {1.0f, 4.0f, 9.0f}, 1u};
    RtxTileState tile = {7u, 0.5f};
    RtxPixelShade out;
    uint8_t rgb[3];
    const RtxAdaptRule ok = {2u, 0.0f};
    const RtxAdaptRule bad[] = {{0u, 0.0f}, {2u, -1.0f}, {2u, std::numeric_limits<float>::quiet_NaN()}, {2u, -inf}};
    CHECK(rtxh_moment_add(1, 1, nullptr, &one, &tile, 0, &ok) == RTX_ERR_BAD_ARG && rtxh_moment_add(1, 1, &s, nullptr, &tile, 0, &ok) == RTX_ERR_BAD_ARG);
    CHECK(rtxh_moment_add(1, 1, &s, &one, &tile, 0, nullptr) == RTX_ERR_BAD_ARG);
    for (const RtxAdaptRule &b : bad) CHECK(rtxh_moment_add(1, 1, &s, &one, &tile, 0, &b) == RTX_ERR_BAD_ARG);
    CHECK(rtxh_moment_add(1u << 14, (1u << 14) + 1u, &s, &one, nullptr, 0, nullptr) == RTX_ERR_BAD_ARG);
    CHECK(rtxh_moment_add(0, 5, nullptr, nullptr, nullptr, 1, nullptr) == RTX_ERR_BAD_ARG);
    CHECK(rtxh_moment_add(0, 5, &s, &one, &tile, 1, &ok) == RTX_OK && rtxh_moment_add(5, 0, &s, &one, nullptr, 1, nullptr) == RTX_OK);
    CHECK(one.frames == 1u && one.sum[0] == 1.0f && tile.frames == 7u && tile.err == 0.5f);
    const RtxAdaptRule any = {2u, inf};
    CHECK(rtxh_moment_add(1, 1, &s, &one, &tile, 0, &any) == RTX_OK);                       // a stopped tile: nothing is touched
    CHECK(one.frames == 1u && one.sum[0] == 1.0f && tile.frames == 7u && tile.err == 0.5f);
    CHECK(rtxh_moment_add(1, 1, &s, &one, nullptr, 0, nullptr) == RTX_OK && one.frames == 2u && tile.frames == 7u);
    CHECK(rtxh_moment_resolve(nullptr, 1, &one, rgb, &out) == RTX_ERR_BAD_ARG && rtxh_moment_resolve(thr, 1, nullptr, rgb, &out) == RTX_ERR_BAD_ARG);
    CHECK(rtxh_moment_resolve(thr, 1, &one, nullptr, nullptr) == RTX_ERR_BAD_ARG && rtxh_moment_resolve(thr, 0, &one, rgb, nullptr) == RTX_OK);
    CHECK(rtxh_moment_resolve(thr, 1, &one, rgb, &out) == RTX_OK && out.linear[0] == (1.0f + 0.3f) / 2.0f && out.hits == 2);

    std::printf("adapt sanitizer driver: %d failed checks\n", fails);
    return fails ? 1 : 0;
}
