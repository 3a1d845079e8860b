"""Fixtures for the tests of the adaptive mean through the render pipeline (rtx_render_view_rows_adaptive,
rtx_render_view_rows_shade_masked_device), with the CPU oracle's answers: numpy and the oracle binding only, no GPU.

The pipeline renders full-width rows, so adapt_sets' ragged rectangles do not apply; these are full-width WINDOWS over
accum_sets' frames under adapt_sets.RULE, 8 frames, through adapt_sets' numpy statements:
    bunny        adapt_sets' own (48 x 32, all rows)
    rows_low     rows [17, 30) of that frame: the bunny and its shadow, a ragged bottom edge (13 rows)
    rows_mid     rows [13, 22): two tile rows, the second one row high
    rows_sky     rows [3, 16): sky only, every tile stops at min_frames
    narrow       rows [11, 27) of a 41 x 27 bunny frame (the same camera recipe and tables): the right column of tiles is one
                 pixel wide
    yard, yard_posed   adapt_sets' own: full width already; two rays per pixel, spheres, a pose
A window's tile rows are the rectangle's, not the frame's: tile (tx, ty) of a window holds rows [y0 + 8 ty, y0 + 8 ty + 8).

The mistake these fixtures must tell from the statement: a scheduling pass that reads a tile's state by the pipeline's own
tile number (tiles numbered within blocks of 8 x 8 tiles: 8 ty + tx for the frames here) where the states are numbered row by
row (tiles_x ty + tx).  run_swizzled() plays it: the launch skips the tiles whose state AT THE WRONG INDEX says stopped, their
scratch records stay the frame before's, and the add — which numbers the tiles as the states are — adds those.  A read past
the states sees what the GPU tests put behind every buffer, bytes of 0xAA: frames = 0xAAAAAAAA and err = -3.03e-13, a stopped
tile under every rule.  With 6 tiles per row the two numberings differ from the second tile row on.
tests/test_rows_adapt_sets.py asserts the conditions; tests/test_gpu_rows_adapt.py uses the fixtures.  Everything is built once
per process (query_sets._once) and read-only."""
import os

import numpy as np

import accum_sets as ac
import adapt_sets as ad
import query_sets as qs
from query_sets import NO_HIT

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NARROW_FRAME = (41, 27)
WINDOWS = {"rows_low": ("bunny", 17, 13), "rows_mid": ("bunny", 13, 9), "rows_sky": ("bunny", 3, 13), "narrow": ("narrow", 11, 16)}
FIXTURES = ("bunny", "rows_low", "rows_mid", "rows_sky", "narrow", "yard", "yard_posed")
# the stop frames (0 = never) of the windows and of the bunny, tile row by tile row, checked with the oracle
STOPS = {"bunny": [[2] * 6, [2] * 6, [0] * 6, [3, 6, 3, 3, 5, 3]],
         "rows_low": [[0] * 6, [3, 4, 3, 3, 3, 3]],
         "rows_mid": [[0] * 6, [2, 3, 2, 2, 3, 2]],
         "rows_sky": [[2] * 6, [2] * 6],
         "narrow": [[0] * 6, [3, 3, 3, 3, 3, 4]]}


def frame_size(fixture):
    if fixture in WINDOWS:
        return ac.BUNNY_FRAME if WINDOWS[fixture][0] == "bunny" else NARROW_FRAME
    return ac.BUNNY_FRAME if fixture == "bunny" else ac.YARD_MEAN_VIEW[0]


def rows_of(fixture):
    """(y0, ny) of the fixture's rows in its frame"""
    if fixture in WINDOWS:
        return WINDOWS[fixture][1:]
    return 0, frame_size(fixture)[1]


def open_narrow(binding, samples):
    """either binding's bunny scene at NARROW_FRAME with `samples` as its table"""
    name = "bunny.obj" if binding.__name__ == "orclib" else os.path.join(ROOT, "models", "bunny.obj")
    return binding.default_scene([name], NARROW_FRAME[0], NARROW_FRAME[1], samples, nb_light_sample=ac.BUNNY_LIGHT_SAMPLES)


def narrow_frame(orc, k):
    def make():
        osc = open_narrow(orc, ac.table(orc, k))
        frame, _, tri, lin = osc.render_rows(mode=orc.MODE_BVH, want_tri=True, want_lin=True)
        osc.close()
        return dict(lin=ac._frozen(lin), hit=ac._frozen(tri != NO_HIT), rgb8=ac._frozen(frame))
    return qs._once("rows_adapt_narrow_%d" % k, make)


def fixture_frames(orc, rtx, fixture, n):
    """(lins, hits) of a fixture's first n oracle frames, cut to its rows"""
    if fixture not in WINDOWS:
        return ad.fixture_frames(orc, rtx, fixture, n)
    base, y0, ny = WINDOWS[fixture]
    fr = ac.frames(orc, rtx, "bunny", n) if base == "bunny" else [narrow_frame(orc, k) for k in range(n)]
    return [f["lin"][y0:y0 + ny] for f in fr], [f["hit"][y0:y0 + ny] for f in fr]


def fixture_rule(fixture):
    return ad.fixture_rule(fixture)


def fixture_count(fixture):
    return ad.fixture_count(fixture)


def view_of(rtx, scene, fixture):
    """the RtxView a call is handed for the fixture on `scene` (the bunny's or the narrow scene's own view cut to the rows;
    the yard's mean view)"""
    if fixture.startswith("yard"):
        return ac.yard_view(rtx)
    v = rtx.rtx.RtxView.from_buffer_copy(scene.own_view())
    y0, ny = rows_of(fixture)
    v.x0, v.y0, v.nx, v.ny = 0, y0, v.width, ny
    return v


def _finish(orc, out):
    out["linear"] = ad.np_divide_own(out["mom"])
    out["rgb8"] = ac.oracle_bytes(orc, out["linear"])
    out["hits"] = np.minimum(out["mom"]["hit_frames"], 255).astype(np.uint8)
    for a in [out["tiles"], out["stop"], out["linear"], out["rgb8"], out["hits"]] + list(out["mom"].values()) + out["history"]:
        a.setflags(write=False)
    return out


def expected(orc, rtx, fixture, n=None, rule=None):
    """adapt_sets.expected for every fixture here: dict(mom, tiles, history, stop, linear, rgb8, hits)"""
    if fixture not in WINDOWS:
        return ad.expected(orc, rtx, fixture, n, rule)
    n = fixture_count(fixture) if n is None else n
    rule = fixture_rule(fixture) if rule is None else rule

    def make():
        lins, hits = fixture_frames(orc, rtx, fixture, n)
        return _finish(orc, ad.run(rule, lins, hits))
    return qs._once("rows_adapt_expected_%s_%d_%r" % (fixture, n, rule), make)


# ---------------------------------------------------------------------------------------------- the two tile numberings
def swizzled_tile_id(tx, ty, tiles_x):
    """the pipeline's number of tile (tx, ty): blocks of 8 x 8 tiles row by row, the tiles of a block numbered consecutively"""
    blocks_x = (tiles_x + 7) // 8
    return (((ty >> 3) * blocks_x + (tx >> 3)) << 6) + ((ty & 7) << 3) + (tx & 7)


def row_major_tile(tx, ty, tiles_x):
    return ty * tiles_x + tx


GUARD_STATE = np.frombuffer(bytes([0xAA]) * 8, ad.TILE_DTYPE)            # what lies behind a guarded buffer of states
GUARD_STATE_STOPPED = True


def run_swizzled(rule, lins, hits):
    """the frames under the rule with the launch's mask read at the pipeline's tile number (the mistake) -> the moments"""
    ny, nx = hits[0].shape
    tx_n, ty_n = ad.tile_grid(nx, ny)
    wrong = np.array([[swizzled_tile_id(tx, ty, tx_n) for tx in range(tx_n)] for ty in range(ty_n)])
    assert ad.np_stopped(rule, GUARD_STATE).all() == GUARD_STATE_STOPPED
    state = None
    scratch_lin = scratch_hit = None
    for lin, hit in zip(lins, hits):
        if state is None:
            scratch_lin, scratch_hit = lin.copy(), hit.copy()
        else:
            flat = state[1].reshape(-1)
            stopped_flat = ad.np_stopped(rule, flat)
            seen_stopped = np.where(wrong < len(flat), stopped_flat[np.minimum(wrong, len(flat) - 1)], GUARD_STATE_STOPPED)
            rendered = ad.tiles_of(~seen_stopped)[:ny, :nx]
            scratch_lin = np.where(rendered[..., None], lin, scratch_lin)
            scratch_hit = np.where(rendered, hit, scratch_hit)
        state = ad.np_frame(rule, scratch_lin, scratch_hit, state)
    return state[0]
