"""What the fixtures of tests/adapt_sets.py must hold for tests/test_gpu_adapt.py to detect an adaptive mean that contracts
its squares, multiplies by a reciprocal, lets lanes outside the rectangle into a tile's maximum, resumes a stopped tile or
divides by the call's frame count — asserted by the oracle and the numpy statements alone, no GPU."""
import importlib

import numpy as np
import pytest

import accum_sets as ac
import adapt_sets as ad
from query_sets import F, bits


@pytest.fixture(scope="module")
def rtx():
    return importlib.import_module("ray-tracer-rust_amd")


def differing(a, b):
    """pixels (or tiles) whose words are not the same bits"""
    d = bits(np.asarray(a, F)) != bits(np.asarray(b, F))
    return d.any(axis=-1) if d.ndim == 3 else d


def all_errors(e):
    return np.array([h["err"] for h in e["history"]])


def margin(e, rule):
    """the smallest relative distance of a tile error of any frame from the rule's threshold"""
    thr = F(rule[1])
    return float((np.abs(all_errors(e).astype(np.float64) - thr) / thr).min())


# ---------------------------------------------------------------------------------------------- the issue's conditions
def test_the_bunny_fixture_meets_the_conditions(orc, rtx):
    e = ad.expected(orc, rtx, "bunny")
    min_frames, n = ad.RULE[0], ad.N_FRAMES
    stop = e["stop"]
    print("stop frames (0 = never):\n%s\nnearest tile error: %.2f %% from the threshold" % (stop, 100 * margin(e, ad.RULE)))
    assert stop.shape == (4, 6) and min_frames == 2 and n == 8 == len(ac.SEEDS)
    assert (stop == min_frames).sum() >= 1
    between = set(int(s) for s in stop.ravel() if min_frames < s < n)
    assert len(between) >= 2, between
    assert (stop == 0).sum() >= 1
    assert margin(e, ad.RULE) >= 0.01
    # a tile's count is its stop frame, or N where it never stopped, and every pixel's count is its tile's
    assert np.array_equal(e["tiles"]["frames"], np.where(stop == 0, n, stop))
    assert np.array_equal(e["mom"]["frames"], ad.tiles_of(e["tiles"]["frames"]))
    # the resolved records differ from the plain mean of 8 inside stopped tiles: a stop that is not final, or a resolve
    # that divides by N, shows
    plain = ac.expected(orc, rtx, "bunny", n)
    stopped = ad.tiles_of(stop != 0)
    diff = differing(e["linear"], plain["linear"])
    print("%d pixels of stopped tiles differ from the plain mean, %d bytes" % ((diff & stopped).sum(), ((e["rgb8"] != plain["rgb8"]).any(axis=-1) & stopped).sum()))
    assert (diff & stopped).sum() >= 10 and not (diff & ~stopped).any()
    assert ((e["rgb8"] != plain["rgb8"]).any(axis=-1) & stopped).sum() >= 1
    with np.errstate(all="ignore"):
        by_n = (e["mom"]["sum"] / F(n)).astype(F)
    assert (differing(e["linear"], by_n) & stopped).sum() >= 10
    # where no tile stops early the statement is the mean's
    same = ad.expected(orc, rtx, "bunny", n, (n, 0.0))
    assert set(same["stop"].ravel().tolist()) <= {0, n} and (same["tiles"]["frames"] == n).all()
    assert np.array_equal(bits(same["mom"]["sum"]), bits(plain["sum"])) and np.array_equal(same["mom"]["hit_frames"], plain["hit_frames"])
    assert np.array_equal(bits(same["linear"]), bits(plain["linear"])) and np.array_equal(same["rgb8"], plain["rgb8"])


def test_a_stop_is_final_and_can_be_told_from_one_that_is_not(orc, rtx):
    """every tile that stops between min_frames and N holds, in every later frame, a pixel that is not black: a tile that
    received one more frame has other sums; and its state keeps the words of the frame it stopped at"""
    e = ad.expected(orc, rtx, "bunny")
    lins, _ = ad.fixture_frames(orc, rtx, "bunny", ad.N_FRAMES)
    late = [(j, i) for j in range(4) for i in range(6) if ad.RULE[0] < e["stop"][j, i] < ad.N_FRAMES]
    assert len(late) >= 4
    for j, i in late:
        s = int(e["stop"][j, i])
        for k in range(s, ad.N_FRAMES):
            assert lins[k][8 * j:8 * j + 8, 8 * i:8 * i + 8].any(), (j, i, k)
            assert e["history"][k][j, i] == e["history"][s - 1][j, i], (j, i, k)
        assert not ad.np_stopped(ad.RULE, e["history"][s - 2])[j, i]
    # min_frames == 1 stops every tile after frame 0 for any threshold: the variance of one frame is exactly 0
    one = ad.expected(orc, rtx, "bunny", 3, (1, 0.0))
    assert (one["stop"] == 1).all() and (bits(one["tiles"]["err"]) == 0).all()
    assert np.array_equal(bits(one["linear"]), bits(lins[0]))


@pytest.mark.parametrize("fixture", ("ragged", "ragged_low", "yard", "yard_posed"))
def test_the_other_fixtures(orc, rtx, fixture):
    e = ad.expected(orc, rtx, fixture)
    rule = ad.fixture_rule(fixture)
    stop = e["stop"]
    print("%s: stop frames\n%s\nnearest tile error: %.2f %% from the threshold" % (fixture, stop, 100 * margin(e, rule)))
    assert stop.shape == (2, 3)
    assert margin(e, rule) >= 0.01
    if fixture == "ragged":
        # the rectangle of the issue: 3 x 2 tiles, ragged right and bottom, two workgroups of four wavefronts; sky only
        x0, y0, nx, ny = ad.RAGGED_RECT
        assert (x0 % 8, y0 % 8, nx % 8, ny % 8) == (5, 3, 3, 5) and (stop == rule[0]).all()
        return
    assert (stop == 0).any() and (stop != 0).any() and len(set(stop.ravel().tolist())) >= 3


def wrapped_tile_error(err):
    """the tile error of a kernel whose lanes past the right edge read their slot y * nx + x all the same: a pixel of the next
    row (nothing past the last record)"""
    ny, nx = err.shape
    width = 8 * ad.tile_grid(nx, ny)[0]
    slots = np.arange(ny)[:, None] * nx + np.arange(width)[None, :]
    flat = np.concatenate([err.reshape(-1), np.zeros(width, F)])
    return ad.np_tile_error(flat[np.minimum(slots, err.size)])


def test_a_tile_maximum_over_lanes_outside_the_rectangle_shows(orc, rtx):
    """in the right-hand column of tiles of the ragged rectangle over the bunny and of the synthetic one, after some frame"""
    shown = {}
    for name, (lins, hits) in (("ragged_low", ad.fixture_frames(orc, rtx, "ragged_low", ad.N_FRAMES)),
                               ("synthetic", ([r["linear"] for r in ad.synthetic(rtx)], [r["hits"] != 0 for r in ad.synthetic(rtx)]))):
        mom, count = None, 0
        for lin, hit in zip(lins, hits):
            mom = ad.np_add(lin, hit, mom)
            err = ad.np_error(mom)
            count += int(differing(wrapped_tile_error(err)[:, -1], ad.np_tile_error(err)[:, -1]).sum())
            assert not differing(wrapped_tile_error(err)[:, :-1], ad.np_tile_error(err)[:, :-1]).any()
        shown[name] = count
    print("tile errors of the last column that differ with the lanes outside: %r" % shown)
    assert shown["ragged_low"] >= 1 and shown["synthetic"] >= 1


# ---------------------------------------------------------------------------------------------- what the fixtures can tell
def test_the_frames_tell_a_contracted_square_and_a_reciprocal_from_the_statement(orc, rtx):
    lins, hits = ad.fixture_frames(orc, rtx, "bunny", ad.N_FRAMES)
    e = ad.expected(orc, rtx, "bunny", ad.N_FRAMES, (ad.N_FRAMES, 0.0))
    # an FMA: sumsq + l * l rounded once
    fused = None
    for lin in lins:
        exact = lin.astype(np.float64) * lin.astype(np.float64)
        fused = exact.astype(F) if fused is None else (fused.astype(np.float64) + exact).astype(F)
    n_fused = int(differing(e["mom"]["sumsq"], fused).sum())
    mutant = dict(e["mom"], sumsq=fused)
    t_fused = int(differing(ad.np_tile_error(ad.np_error(mutant)), e["tiles"]["err"]).sum())
    # a reciprocal in place of each division
    fn = F(ad.N_FRAMES - 1)                                            # 8 is a power of two: its reciprocal is exact
    seven = ad.expected(orc, rtx, "bunny", ad.N_FRAMES - 1, (ad.N_FRAMES, 0.0))
    with np.errstate(all="ignore"):
        r = F(1.0) / fn
        mean = (seven["mom"]["sum"] * r).astype(F)
        v = ((seven["mom"]["sumsq"] * r).astype(F) - (mean * mean).astype(F)).astype(F)
        err = (np.where(v > 0, v, F(0.0)).astype(F) * r).astype(F).max(axis=-1)
    n_recip = int(differing(seven["linear"], mean).sum())
    t_recip = int(differing(ad.np_tile_error(err), seven["tiles"]["err"]).sum())
    print("%d pixels' sumsq differ fused (%d tile errors), %d quotients differ from the reciprocal product (%d tile errors)"
          % (n_fused, t_fused, n_recip, t_recip))
    assert n_fused >= 10 and t_fused >= 1 and n_recip >= 10 and t_recip >= 1


def test_the_synthetic_frames_hold_what_no_render_produces(rtx):
    syn = ad.synthetic(rtx)
    ny, nx = ad.SYNTHETIC_SHAPE
    assert syn[0].shape == (ny, nx) and nx % 8 and ny % 8 and ad.tile_grid(nx, ny) == (5, 4)
    lin0 = syn[0]["linear"]
    for value in (-0.0, 1e-45, 1e-40, 2.0 ** 61, 2.0 ** -61, np.inf, -np.inf):
        assert (bits(lin0) == bits(np.array([value], F))[0]).any(), value
    assert np.isnan(lin0).any() and set(np.unique(syn[0]["hits"])) >= {0, 1, 255}
    r = ad.synthetic_run(rtx)
    err = all_errors(r)
    assert not np.isnan(err).any() and (err >= 0).all()                # never NaN, never negative, whatever the records hold
    assert np.isinf(r["mom"]["sumsq"]).any() and np.isnan(r["mom"]["sum"]).any()
    # the squares of 2^61 are about 5e36: under a threshold of 1e36 some tiles stop at min_frames and others later; under
    # +infinity, which a rule may name, all stop at min_frames; under a threshold of 1 none ever stops
    print("synthetic stop frames\n%s\nnearest tile error: %.2f %% from the threshold" % (r["stop"], 100 * margin(r, ad.SYNTHETIC_RULE)))
    assert len(set(r["stop"].ravel().tolist())) >= 2 and (r["stop"] == ad.SYNTHETIC_RULE[0]).any() and margin(r, ad.SYNTHETIC_RULE) >= 0.01
    assert (ad.synthetic_run(rtx, (3, np.inf))["stop"] == 3).all()
    never = ad.synthetic_run(rtx, (2, 1.0))
    assert (never["stop"] == 0).all() and (never["mom"]["frames"] == ac.SYNTHETIC_FRAMES).all()
