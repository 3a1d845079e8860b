"""What the fixtures of tests/rows_adapt_sets.py must hold for tests/test_gpu_rows_adapt.py to detect a masked scheduling pass
that reads a tile's state by the pipeline's own tile number, stops too early or too late, or resumes a stopped tile — asserted
by the oracle and the numpy statements alone, no GPU."""
import importlib

import numpy as np
import pytest

import accum_sets as ac
import adapt_sets as ad
import rows_adapt_sets as ra
from query_sets import F, bits


@pytest.fixture(scope="module")
def rtx():
    return importlib.import_module("ray-tracer-rust_amd")


def margin(e, rule):
    """the smallest relative distance of a tile error of any frame, other than an exact 0, from the rule's threshold"""
    thr = F(rule[1])
    errs = np.array([h["err"] for h in e["history"]]).astype(np.float64)
    return float((np.abs(errs - thr) / thr).min())


def moments_differ(a, b):
    return any(not np.array_equal(bits(np.asarray(a[k], F)) if a[k].dtype == F else a[k], bits(np.asarray(b[k], F)) if b[k].dtype == F else b[k])
               for k in ("sum", "sumsq", "hit_frames", "frames"))


WINDOW_MARGINS = {"bunny": 0.030, "rows_low": 0.027, "rows_mid": 0.10, "narrow": 0.025}      # as measured with the oracle


@pytest.mark.parametrize("fixture", ("bunny", "rows_low", "rows_mid", "rows_sky", "narrow"))
def test_the_windows_stop_where_stated(orc, rtx, fixture):
    e = ra.expected(orc, rtx, fixture)
    rule, n = ra.fixture_rule(fixture), ra.fixture_count(fixture)
    (w, h), (y0, ny) = ra.frame_size(fixture), ra.rows_of(fixture)
    assert rule == ad.RULE and n == ad.N_FRAMES == 8 and y0 + ny <= h
    assert e["mom"]["frames"].shape == (ny, w) and e["stop"].shape == ad.tile_grid(w, ny)[::-1]
    print("%s: stop frames (0 = never)\n%s" % (fixture, e["stop"]))
    assert e["stop"].tolist() == ra.STOPS[fixture]
    assert np.array_equal(e["tiles"]["frames"], np.where(e["stop"] == 0, n, e["stop"]))
    assert np.array_equal(e["mom"]["frames"], ad.tiles_of(e["tiles"]["frames"])[:ny, :w])
    if fixture == "rows_sky":
        assert (e["stop"] == rule[0]).all() and not e["mom"]["hit_frames"].any()
        return
    m = margin(e, rule)
    print("nearest tile error: %.2f %% from the threshold" % (100 * m))
    assert (e["stop"] == 0).any()                                       # a tile that never stops
    assert (e["stop"] > rule[0]).any()                                  # ... and one that stops after min_frames
    assert m >= 0.02
    assert abs(m - WINDOW_MARGINS[fixture]) <= 0.1 * WINDOW_MARGINS[fixture]
    # the states read by the pipeline's own tile number give other moments
    lins, hits = ra.fixture_frames(orc, rtx, fixture, n)
    wrong = ra.run_swizzled(rule, lins, hits)
    assert moments_differ(wrong, e["mom"]), fixture


def test_the_narrow_frames_right_column_is_one_pixel_wide(orc, rtx):
    w, h = ra.NARROW_FRAME
    assert w % 8 == 1 and ad.tile_grid(w, ra.rows_of("narrow")[1]) == (6, 2)
    e = ra.expected(orc, rtx, "narrow")
    assert e["stop"][1, 5] == 4 and e["stop"][1, 4] == 3                # the one-pixel column decides for itself


def test_the_two_tile_numberings(orc, rtx):
    """they agree on the first tile row and nowhere else for 6 tiles per row; on a 9 x 9 grid the pipeline's number crosses
    a block of 8 in both directions"""
    assert [ra.swizzled_tile_id(tx, 0, 6) for tx in range(6)] == [ra.row_major_tile(tx, 0, 6) for tx in range(6)]
    assert all(ra.swizzled_tile_id(tx, ty, 6) != ra.row_major_tile(tx, ty, 6) for ty in range(1, 4) for tx in range(6))
    ids = sorted(ra.swizzled_tile_id(tx, ty, 9) for ty in range(9) for tx in range(9))
    assert len(set(ids)) == 81 and ids[63] == 63 and ids[64] == 64 and ids[-1] == 192 and max(ids) < 4 * 64
    assert ra.swizzled_tile_id(8, 0, 9) == 64 and ra.swizzled_tile_id(0, 8, 9) == 128 and ra.swizzled_tile_id(8, 8, 9) == 192


@pytest.mark.parametrize("fixture", ("yard", "yard_posed"))
def test_the_yards_are_full_width_already(orc, rtx, fixture):
    """adapt_sets' own: two rays per pixel, spheres, a pose; tiles that stop and tiles that do not"""
    e = ra.expected(orc, rtx, fixture)
    (w, h), (y0, ny) = ra.frame_size(fixture), ra.rows_of(fixture)
    assert (y0, ny) == (0, h) and e["mom"]["frames"].shape == (h, w)
    assert ra.fixture_rule(fixture) == ad.YARD_RULE and ra.fixture_count(fixture) == ac.YARD_FRAMES
    assert (e["stop"] == 0).any() and (e["stop"] != 0).any()
