"""What the fixtures of tests/resample_sets.py must hold for tests/test_gpu_resample.py to detect an implementation that
ignores a new table, or applies only its jitter half or only its light half — asserted by the oracle alone, no GPU — and the
one statement of a seeded table against the two generators."""
import importlib

import numpy as np
import pytest

import prims_sets as pm
import resample_sets as rs
from query_sets import bits


@pytest.fixture(scope="module")
def rtx():
    return importlib.import_module("ray-tracer-rust_amd")


def test_the_tables_are_what_they_are_for(orc):
    t = rs.tables(orc)
    a, at = t["A"], rs.light_indices(rs.N_A)
    assert at == list(range(12)) and len(a) == rs.N_A
    elsewhere = np.ones(rs.N_A, bool)
    elsewhere[at] = False
    assert np.array_equal(bits(t["B"][at]), bits(a[at])) and (bits(t["B"][elsewhere]) != bits(a[elsewhere])).all(axis=1).all()
    assert np.array_equal(bits(t["C"][elsewhere]), bits(a[elsewhere])) and (bits(t["C"][at]) != bits(a[at])).all(axis=1).all()
    w, h = rs.YARD_FRAME
    assert len(t["D7"]) == 7 < pm.NB_LIGHT < w * h and len(t["D1"]) == 1 and len(t["Dbig"]) == rs.GROWN_PAIRS > rs.N_A
    for name, seed in rs.SEED_OF.items():
        assert len(t[name]) == rs.SEEDED_PAIRS and rs.SEEDED_PAIRS % 2 == 1
        assert np.array_equal(bits(t[name]), bits(orc.gen_samples(seed, rs.SEEDED_PAIRS)))
    assert (t["half"] == 0.5).all()
    assert np.isinf(t["inf"][3, 0]) and 3 in at and np.array_equal(bits(t["inf"][4:]), bits(a[4:]))
    assert set(rs.RENDERED) == set(t) - {"A", "inf"}


def test_every_table_changes_the_yards_frame(orc, rtx, samples_seeded):
    """a resample that does nothing fails on every table; B moves the primary rays alone and C the light points alone, and
    each changes bytes: an implementation that applies one half only fails on the other"""
    own = rs.yard_render(orc, rtx, samples_seeded, "A")
    assert own["stats"]["primary_hits"] > 300
    for name in rs.RENDERED:
        r = rs.yard_render(orc, rtx, samples_seeded, name)
        changed = int((r["frame"] != own["frame"]).any(axis=2).sum())
        print("%s: %d of %d pixels differ from A's frame" % (name, changed, own["frame"].shape[0] * own["frame"].shape[1]))
        assert changed > 0, name
    # B's light points are A's (the table entries they are made from are): its pixels differ by the primary rays alone.
    # C's primary rays are A's but for the few that read one of the twelve entries, and pixels whose rays are A's change
    # bytes: the light points alone
    b, c = (rs.yard_render(orc, rtx, samples_seeded, n) for n in ("B", "C"))
    w, h = rs.YARD_FRAME
    moved = lambda r: (bits(r["rays"][1]) != bits(own["rays"][1])).any(axis=1).reshape(h, w, pm.NB_RAY).any(axis=2)
    assert moved(b).sum() > w * h - 12 and moved(c).sum() <= 12
    still = ~moved(c)
    assert np.array_equal(c["tri"][still], own["tri"][still]) and (c["frame"][still] != own["frame"][still]).any()
    # ... and under the fixture light and for every pose that stands through a resample
    for name in ("B", "C", "seed_1"):
        lit_own, lit = (rs.yard_render(orc, rtx, samples_seeded, n, light=rs.YARD_LIGHT) for n in ("A", name))
        assert (lit["frame"] != lit_own["frame"]).any(), name
        assert (lit["frame"] != rs.yard_render(orc, rtx, samples_seeded, name)["frame"]).any(), name
        for pose in rs.POSES:
            p_own, p = (rs.yard_render(orc, rtx, samples_seeded, n, pose=pose) for n in ("A", name))
            assert (p["frame"] != p_own["frame"]).any(), (name, pose)
            assert (p["frame"] != rs.yard_render(orc, rtx, samples_seeded, name)["frame"]).any(), (name, pose)


def test_every_table_changes_the_bunnys_frame(orc):
    own, lit_own = rs.bunny_render(orc, "A"), rs.bunny_render(orc, "A", lit=True)
    assert (own["frame"] != lit_own["frame"]).any()
    for name in rs.BUNNY_TABLES:
        assert (rs.bunny_render(orc, name)["frame"] != own["frame"]).any(), name
        assert (rs.bunny_render(orc, name, lit=True)["frame"] != lit_own["frame"]).any(), name


def test_the_statement_is_both_generators(orc, rtx):
    """sample_statement's closed form (resample_sets.stated, and the library's own compilation of it behind
    rtx_scene_samples on a seeded scene) against rtxh_gen_samples' and orc_gen_samples' running sums: a whole 2,000,000-pair
    table for every seed, once"""
    with rs.open_yard(rtx, rs.tables(orc)["A"]) as scene:
        for seed in rs.SEEDS:
            want = rtx.gen_samples(seed, rs.WHOLE_PAIRS)
            assert np.array_equal(bits(want), bits(orc.gen_samples(seed, rs.WHOLE_PAIRS))), seed
            assert np.array_equal(bits(rs.stated(seed, 0, rs.WHOLE_PAIRS)), bits(want)), seed
            scene.reseed(seed, rs.WHOLE_PAIRS)
            assert np.array_equal(bits(scene.samples_at()), bits(want)), seed
            assert (want >= 0).all() and (want < 1).all()
