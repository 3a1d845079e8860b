"""Fixtures for the tests of the adaptive mean of N frames (rtx_render_view_adaptive, rtx_moment_add_device,
rtx_moment_resolve_device, rtxh_moment_add, rtxh_moment_resolve), with the CPU oracle's answers: numpy, the oracle binding and
the library's host side only, no GPU.

The frames are accum_sets' — frame k is the ORACLE SCENE CREATED WITH THE TABLE gen_samples(SEEDS[k], N_PAIRS), rendered whole
— and the four statements are stated here once more, in numpy float32 (every operation one rounding, products rounded before
they are added or subtracted):
    np_add       moment_add_statement over the pixels of the live tiles
    np_error     moment_error_statement per pixel
    np_tiles     the tile error (the maximum over the pixels inside the rectangle, from +0.0) and the tile's frame count
    np_stopped   tile_stopped
    np_resolve   moment_resolve_statement: every pixel divided by its own count
run() plays a sequence of frames through them under a rule and returns the moments, the tile states after every frame, the
stop frames and the resolved records; expected() is run() over a fixture's oracle frames, with the oracle's bytes.

Fixtures:
    bunny        accum_sets' bunny, 48 x 32, 8 frames, RULE: tiles stop at min_frames, at several frames in between and never
    ragged       RAGGED_RECT of that frame: x0 = 5, y0 = 3, 19 x 13 — 3 x 2 tiles, ragged right and bottom, two workgroups of
                 four wavefronts
    ragged_low   RAGGED_LOW_RECT, the same shape 14 rows lower, where the bunny and its shadow are: the issue's rectangle holds
                 sky only (every tile stops at min_frames), this one tiles that stop at 3, at 4 and never
    yard         accum_sets' yard (two rays per pixel, spheres), 3 frames, YARD_RULE
    yard_posed   the same under the pose
and accum_sets' synthetic records (what no render produces) as frames of a SYNTHETIC_SHAPE rectangle.
tests/test_adapt_sets.py asserts, without a GPU, the conditions the fixtures must meet and that they tell the statement from
its likely mistakes; tests/test_adapt_host.py and tests/test_gpu_adapt.py use them.  Everything is built once per process
(query_sets._once) and read-only."""
import numpy as np

import accum_sets as ac
import query_sets as qs
from query_sets import F

N_FRAMES = 8
RULE = (2, float(F(3e-6)))                   # (min_frames, max_variance)
RAGGED_RECT = (5, 3, 19, 13)                 # x0, y0, nx, ny of the bunny's frame
RAGGED_LOW_RECT = (5, 17, 19, 13)            # the same shape over the bunny and its shadow: tiles that stop late or never
YARD_RULE = (2, float(F(0.0254)))            # 7 % from the nearest tile error of either yard fixture (measured with the oracle)
SYNTHETIC_SHAPE = (27, 37)                   # ny, nx: 999 of accum_sets' 1031 synthetic records, 4 x 5 ragged tiles
SYNTHETIC_RULE = (2, float(F(1e36)))         # among the tile errors the squares of 2^61 make


TILE_DTYPE = np.dtype([("frames", np.uint32), ("err", np.float32)])


def tile_grid(nx, ny):
    return (nx + 7) // 8, (ny + 7) // 8


def tiles_of(a):
    """[ny, nx] per tile -> [8 * tiles_y, 8 * tiles_x] per pixel"""
    return np.repeat(np.repeat(a, 8, axis=0), 8, axis=1)


# ---------------------------------------------------------------------------------------------- the statements in numpy
def np_add(lin, hit, mom=None, live=None):
    """moment_add_statement over arrays: lin float32 [ny, nx, 3], hit bool [ny, nx]; mom: None (first) or the dict np_add
    returns (not modified); live: bool [ny, nx], the pixels whose tile receives the frame (None: all)"""
    lin = lin.astype(F)
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        sq = (lin * lin).astype(F)
        if mom is None:
            return dict(sum=lin.copy(), hit_frames=hit.astype(np.uint32), sumsq=sq, frames=np.ones(hit.shape, np.uint32))
        new = dict(sum=(mom["sum"] + lin).astype(F), hit_frames=(mom["hit_frames"] + hit.astype(np.uint32)).astype(np.uint32),
                   sumsq=(mom["sumsq"] + sq).astype(F), frames=(mom["frames"] + np.uint32(1)).astype(np.uint32))
    if live is None:
        return new
    return {k: np.where(live[..., None] if new[k].ndim == 3 else live, new[k], mom[k]) for k in new}


def np_error(mom):
    """moment_error_statement per pixel -> float32 [ny, nx], never NaN, never negative"""
    with np.errstate(all="ignore"):
        fn = mom["frames"].astype(F)[..., None]
        mean = (mom["sum"] / fn).astype(F)
        q = (mom["sumsq"] / fn).astype(F)
        v = (q - (mean * mean).astype(F)).astype(F)
        v = np.where(v > 0, v, F(0.0)).astype(F)
        e = (v / fn).astype(F)
    out = np.where(e[..., 0] < e[..., 1], e[..., 1], e[..., 0])
    return np.where(out < e[..., 2], e[..., 2], out).astype(F)


def np_tile_error(err):
    """the tile error: the maximum over the tile's pixels inside the rectangle, starting from +0.0"""
    ny, nx = err.shape
    tx, ty = tile_grid(nx, ny)
    out = np.zeros((ty, tx), F)
    for j in range(ty):
        for i in range(tx):
            out[j, i] = max(F(0.0), err[8 * j:8 * j + 8, 8 * i:8 * i + 8].max())
    return out


def np_stopped(rule, tiles):
    with np.errstate(invalid="ignore"):
        return (tiles["frames"] >= rule[0]) & (tiles["err"] <= F(rule[1]))


def np_divide_own(mom):
    with np.errstate(all="ignore"):
        return (mom["sum"] / mom["frames"].astype(F)[..., None]).astype(F)


def np_resolve(rtx, thr, mom):
    linear = np_divide_own(mom)
    return ac.as_records(rtx, linear, ac.np_bytes(thr, linear), np.minimum(mom["hit_frames"], 255).astype(np.uint8))


def np_frame(rule, lin, hit, state=None):
    """one frame through the statements: state None (first) or (mom, tiles) -> (mom, tiles), new arrays"""
    ny, nx = hit.shape
    if state is None:
        mom = np_add(lin, hit)
        tiles = np.zeros(tile_grid(nx, ny)[::-1], TILE_DTYPE)
        live_tiles = np.ones(tiles.shape, bool)
    else:
        mom, tiles = state
        live_tiles = ~np_stopped(rule, tiles)
        mom = np_add(lin, hit, mom, tiles_of(live_tiles)[:ny, :nx])
        tiles = tiles.copy()
    err = np_tile_error(np_error(mom))
    tiles["frames"] = np.where(live_tiles, tiles["frames"] + 1, tiles["frames"])
    tiles["err"] = np.where(live_tiles, err, tiles["err"])
    return mom, tiles


def run(rule, lins, hits, state=None):
    """the frames, in order, under the rule -> dict(mom, tiles, history: the tile states after every frame, stop: the frame
    count at which each tile stopped, 0 = never)"""
    history = []
    for lin, hit in zip(lins, hits):
        state = np_frame(rule, lin, hit, state)
        history.append(state[1])
    mom, tiles = state
    stop = np.where(np_stopped(rule, tiles), tiles["frames"], 0).astype(np.uint32)
    return dict(mom=mom, tiles=tiles, history=history, stop=stop)


# ---------------------------------------------------------------------------------------------- the fixtures
def fixture_frames(orc, rtx, fixture, n):
    """(lins, hits) of a fixture's first n oracle frames, cut to its rectangle"""
    if fixture in ("ragged", "ragged_low"):
        x0, y0, nx, ny = RAGGED_RECT if fixture == "ragged" else RAGGED_LOW_RECT
        fr = ac.frames(orc, rtx, "bunny", n)
        return [f["lin"][y0:y0 + ny, x0:x0 + nx] for f in fr], [f["hit"][y0:y0 + ny, x0:x0 + nx] for f in fr]
    fr = ac.frames(orc, rtx, fixture, n)
    return [f["lin"] for f in fr], [f["hit"] for f in fr]


def fixture_rule(fixture):
    return YARD_RULE if fixture.startswith("yard") else RULE


def fixture_count(fixture):
    return ac.YARD_FRAMES if fixture.startswith("yard") else N_FRAMES


def expected(orc, rtx, fixture, n=None, rule=None):
    """run() over the fixture's oracle frames and the resolved records: dict(mom, tiles, history, stop, linear float32
    [ny, nx, 3], rgb8 uint8 [ny, nx, 3] by the oracle's Color::to_rgba, hits uint8 [ny, nx])"""
    n = fixture_count(fixture) if n is None else n
    rule = fixture_rule(fixture) if rule is None else rule

    def make():
        lins, hits = fixture_frames(orc, rtx, fixture, n)
        out = run(rule, lins, hits)
        out["linear"] = np_divide_own(out["mom"])
        out["rgb8"] = ac.oracle_bytes(orc, out["linear"])
        out["hits"] = np.minimum(out["mom"]["hit_frames"], 255).astype(np.uint8)
        for a in [out["tiles"], out["stop"], out["linear"], out["rgb8"], out["hits"]] + list(out["mom"].values()) + out["history"]:
            a.setflags(write=False)
        return out
    return qs._once("adapt_expected_%s_%d_%r" % (fixture, n, rule), make)


def as_moments(rtx, mom):
    out = np.zeros(mom["frames"].shape, rtx.MOMENT_PIXEL_DTYPE)
    for k in ("sum", "hit_frames", "sumsq", "frames"):
        out[k] = mom[k]
    return out


def same_words(got, want):
    """float words equal bit for bit, a NaN standing for any NaN"""
    nan = np.isnan(want)
    return np.array_equal(np.isnan(got), nan) and np.array_equal(qs.bits(got)[~nan], qs.bits(want)[~nan])


def same_moments(got, mom):
    """a MOMENT_PIXEL_DTYPE array against np_add's dict, word for word"""
    return (same_words(got["sum"], mom["sum"]) and same_words(got["sumsq"], mom["sumsq"])
            and np.array_equal(got["hit_frames"], mom["hit_frames"]) and np.array_equal(got["frames"], mom["frames"]))


def same_tiles(got, want):
    return np.array_equal(got["frames"], want["frames"]) and np.array_equal(qs.bits(got["err"]), qs.bits(want["err"]))


# ---------------------------------------------------------------------------------------------- synthetic records
def synthetic(rtx):
    """accum_sets' synthetic frames as rectangles of SYNTHETIC_SHAPE"""
    ny, nx = SYNTHETIC_SHAPE
    return [rec[:ny * nx].reshape(ny, nx) for rec in ac.synthetic(rtx)]


def synthetic_run(rtx, rule=SYNTHETIC_RULE, n_frames=ac.SYNTHETIC_FRAMES):
    syn = synthetic(rtx)[:n_frames]
    return run(rule, [r["linear"] for r in syn], [r["hits"] != 0 for r in syn])
