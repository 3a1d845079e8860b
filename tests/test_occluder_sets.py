"""The conditions the fixtures of tests/occluder_sets.py must meet to test what they are for, stated from the CPU oracle
and numpy alone (no GPU): which verdict the walk's distance certificate gives on each fixture's candidates, and that the
oracle answers both ways where it gives none."""
import numpy as np
import pytest

import occluder_sets as oc


@pytest.fixture(scope="module")
def rays(orc, samples_seeded):
    return {name: oc.shadow_rays(orc, samples_seeded, name) for name in oc.FIXTURES}


def verdicts(s, pick):
    yes, no = oc.certificate(s["origins"][pick], s["t"][pick], s["limit"][pick])
    assert not (yes & no).any()
    return yes, no


@pytest.mark.parametrize("name", oc.FIXTURES)
def test_the_float32_restatement_is_the_oracles_answer(rays, name):
    """main.rs:220-221 on the oracle's closest hit, restated with the hit's t (p_hit = orig + t * dir, bvh.rs:69)"""
    s = rays[name]
    hit = s["prim"] != oc.NO_HIT
    assert hit.sum() >= 200
    got = oc.exact_occludes(s["origins"][hit], s["unit"][hit], s["t"][hit], s["limit"][hit])
    assert np.array_equal(got.astype(np.uint8), s["occluded"][hit])
    assert not s["occluded"][~hit].any()


def test_below_every_candidate_is_a_certified_occluder(rays):
    s = rays["below"]
    hit = s["prim"] != oc.NO_HIT
    assert hit.sum() >= 2000 and (~hit).sum() >= 2000, "the sheet's shadow and the open wall"
    yes, no = verdicts(s, hit)
    assert yes.all() and s["occluded"][hit].all()
    assert (s["t"][hit] * 2.0 < s["limit"][hit]).all(), "far below the light: under half its distance"
    lit = s["image"].max(axis=2) > 0
    assert 100 <= (~lit).sum() and 400 <= lit.sum()


def test_beyond_every_candidate_is_certified_not_to_occlude(rays):
    s = rays["beyond"]
    hit = s["prim"] != oc.NO_HIT
    assert hit.all() and len(hit) == 32 * 32 * oc.NB_LIGHT, "every shadow ray meets the triangle behind the light"
    yes, no = verdicts(s, hit)
    assert no.all() and not s["occluded"].any()
    assert (s["image"].max(axis=2) > 0).all(), "every sample is lit"


@pytest.mark.parametrize("name", ["coplanar", "tile"])
def test_candidates_within_ulps_of_the_lights_distance(rays, name):
    """candidates on the triangle in the light's plane: at least a quarter undecided, and among the undecided rays the
    oracle answers both ways"""
    s = rays[name]
    cand, t = oc.candidates_on(oc.COVER, s["origins"], s["unit"])
    assert cand.sum() >= (2000 if name == "coplanar" else 300)
    yes, no = oc.certificate(s["origins"][cand], t[cand], s["limit"][cand])
    undecided = ~yes & ~no
    assert undecided.sum() * 4 >= cand.sum()
    assert (np.abs(t[cand] - s["limit"][cand]) <= 8 * np.spacing(s["limit"][cand])).all()
    closest_is_cover = cand & (s["prim"] == (0 if name == "coplanar" else 24))
    yes, no = verdicts(s, closest_is_cover)
    answers = s["occluded"][closest_is_cover][~yes & ~no]
    assert (answers == 1).sum() >= 20 and (answers == 0).sum() >= 20


def test_tile_holds_settled_and_unsettled_rays_per_light_point(rays):
    """one 8 x 8 tile: the 64 rays towards each light point (a wavefront of the shading pass) hold candidates the
    certificate settles (on the sheet) and candidates it does not (on the triangle in the light's plane)"""
    s = rays["tile"]
    assert s["fixture"]["W"] == s["fixture"]["H"] == 8 and len(s["origins"]) == 64 * oc.NB_LIGHT
    hit = s["prim"] != oc.NO_HIT
    yes, no = oc.certificate(s["origins"], s["t"], s["limit"])
    settled, unsettled = hit & (yes | no), hit & ~yes & ~no
    on_sheet = hit & (s["prim"] < 24)
    assert (settled[on_sheet]).all() and on_sheet.sum() >= 100
    for k in range(oc.NB_LIGHT):
        assert settled[k::oc.NB_LIGHT].sum() >= 10 and unsettled[k::oc.NB_LIGHT].sum() >= 10, "light point %d" % k
    lit = s["image"].max(axis=2) > 0
    assert lit.any() and (~lit).any()
