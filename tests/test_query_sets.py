"""The conditions the ray sets of tests/query_sets.py must meet to test what they are for, checked with the CPU oracle
alone.  They are conditions on the inputs: a set that misses one gets another seed or size, not a lower threshold.
Each test prints the counts it asserts on (pytest -s)."""
import numpy as np
import pytest

import query_sets as qs
from query_sets import F, NO_HIT


@pytest.fixture(scope="module")
def sets(orc, samples_seeded):
    return lambda name: getattr(qs, name)(orc, samples_seeded)


def outcomes(occ):
    return int(occ.sum()), int((occ == 0).sum())


def test_set_a_mixed_soup_with_spheres(sets):
    a = sets("scene_a")
    o, d, exp, _ = sets("set_a")["trace"]
    _, t, _, occ = sets("set_a")["occlusion"]
    assert len(o) == 1000 and (o >= a["lo"]).all() and (o <= a["hi"]).all() and (t >= a["lo"]).all() and (t <= a["hi"]).all()
    hit, sphere = exp["prim"] != NO_HIT, qs.is_sphere(a, exp)
    inside = qs.inside_a_sphere(a, o)
    print("A: %d hits, %d on spheres; %d occluded, %d lit; %d occluded by a sphere; %d origins inside a sphere"
          % (hit.sum(), sphere.sum(), *outcomes(occ), (sphere & (occ == 1)).sum(), inside.sum()))
    assert sphere.sum() >= 200 and (hit & ~sphere).sum() >= 200
    assert occ.sum() >= 100 and (occ == 0).sum() >= 100
    assert (sphere & (occ == 1)).sum() >= 100
    assert inside.sum() >= 20
    assert np.isfinite(exp["t"]).all()
    assert (hit & inside).sum() >= 20          # sphere_distance's t0 < 0 -> t1 arm decides some answers


def test_set_b_far_origins(sets):
    a, b = sets("scene_a"), sets("set_b")
    o, _, exp, _ = b["far"]["trace"]
    occ = b["far"]["occlusion"][3]
    assert len(o) == 200
    hit, sphere = exp["prim"] != NO_HIT, qs.is_sphere(a, exp)
    print("B: %d hits, %d on spheres, %d occluded" % (hit.sum(), sphere.sum(), occ.sum()))
    assert hit.sum() >= 100 and sphere.sum() >= 30 and occ.sum() >= 50
    assert (np.abs(o).max(axis=1) > a["bound"]).all() and np.isfinite(exp["t"]).all()
    mo, _, mexp, _ = b["mixed"]["trace"]
    near = sets("set_a")["trace"]
    assert len(mo) == 400 and np.array_equal(mo[0::2], o) and np.array_equal(mo[1::2], near[0][:200])
    assert mexp[0::2].tobytes() == exp.tobytes() and mexp[1::2].tobytes() == near[2][:200].tobytes()
    assert (np.abs(mo[1::2]).max(axis=1) <= a["bound"]).all()          # every group of 64 mixes the two kinds of origin


@pytest.mark.parametrize("axis", ["x", "y", "z"])
def test_set_c_a_hard_ray_is_answered_differently_from_its_twin(orc, sets, axis):
    """Each hard ray of the bunny batch has exactly one -0.0 component, and the oracle answers it (a miss: an ancestor
    box of the reference's tree rejects it) differently from the same ray with +0.0 there (a hit on the mesh)."""
    c, osc = sets("set_c")["bunny"], sets("bunny")["osc"]
    slot = qs.HARD_SLOTS[axis]
    o, d, exp, _ = c["trace"]
    negative_zero = (d[slot] == 0) & np.signbit(d[slot])
    assert negative_zero.tolist() == [k == axis for k in "xyz"]
    assert exp["prim"][slot] == NO_HIT
    twin, _ = qs.oracle_hits(orc, osc, o[slot:slot + 1], qs.positive_twin(d[slot])[None], qs.HIT_DTYPE)
    assert twin["prim"][0] == qs.HARD_TWIN_HITS[axis]
    # the occlusion pair keeps the -0.0 through target - origin
    oo, ot, _, _ = c["occlusion"]
    v = (ot[slot] - oo[slot]).astype(F)
    assert ((v == 0) & np.signbit(v)).tolist() == negative_zero.tolist()


def test_set_c_groups(sets):
    c, a, b = sets("set_c"), sets("scene_a"), sets("bunny")
    o, d, exp, _ = c["bunny"]["trace"]
    hard = ((d == 0) & np.signbit(d)).any(axis=1)
    assert len(o) == 150 and np.nonzero(hard)[0].tolist() == [0, 127, 149]
    oo, ot, _, occ = c["bunny"]["occlusion"]
    v = (ot - oo).astype(F)
    assert np.nonzero(((v == 0) & np.signbit(v)).any(axis=1))[0].tolist() == [0, 127, 149]
    assert 0 < occ.sum() < 150
    # the other 147 are the random set's
    keep = ~hard
    assert exp[keep].tobytes() == b["sets"]["random"][2][:150][keep].tobytes()

    o, d, exp, _ = c["scene_a"]["trace"]
    hard = ((d == 0) & np.signbit(d)).any(axis=1)
    assert len(o) == 64 and np.nonzero(hard)[0].tolist() == [63]
    others = int(qs.is_sphere(a, exp)[:63].sum())
    oo, ot, _, occ = c["scene_a"]["occlusion"]
    v = (ot - oo).astype(F)
    assert np.nonzero(((v == 0) & np.signbit(v)).any(axis=1))[0].tolist() == [63]
    print("C: on scene A %d of the 63 regular rays hit a sphere, the hard ray hits %d; %d of 64 pairs occluded"
          % (others, exp["prim"][63], occ.sum()))
    assert others >= 10 and 0 < occ.sum() < 64

    o, d, exp, _ = c["both"]["trace"]
    hard = ((d == 0) & np.signbit(d)).any(axis=1)
    far = np.abs(o).max(axis=1) > 10000.0           # the ground reaches +-10,000: the scene's bound
    assert len(o) == 64 and np.nonzero(hard)[0].tolist() == [40] and np.nonzero(far)[0].tolist() == [17]
    assert exp["prim"][17] != NO_HIT
    oo, ot, _, occ = c["both"]["occlusion"]
    v = (ot - oo).astype(F)
    assert np.nonzero(((v == 0) & np.signbit(v)).any(axis=1))[0].tolist() == [40]
    assert np.nonzero(np.abs(oo).max(axis=1) > 10000.0)[0].tolist() == [17] and 0 < occ.sum() < 64


@pytest.mark.parametrize("scene", ["bunny", "scene_a"])
def test_set_d_occlusion_at_the_edge(sets, scene):
    """The target on the hit point or one ulp from it: distance(origin, p_hit) and the distance to the target are equal
    or an ulp apart, and both outcomes occur in each of the three target arrays."""
    d = sets("set_d")[scene]
    first = d["first_prim"]
    if scene == "bunny":
        off_ground = int((first != sets("bunny")["ground"]).sum())
        print("D %s: %d rays, %d on the mesh" % (scene, len(first), off_ground))
        assert off_ground >= 100                     # the walk has a farther surface of the mesh to meet first
    else:
        kinds = sets("scene_a")["kinds"][first]
        print("D %s: %d rays, %d on spheres" % (scene, len(first), (kinds == 1).sum()))
        assert (kinds == 1).sum() >= 100 and (kinds == 0).sum() >= 100
    for name, (o, t, exp, occ) in d["targets"].items():
        assert len(o) == len(first)
        print("D %s %s: %d occluded, %d lit" % ((scene, name) + outcomes(occ)))
        assert occ.sum() >= 50 and (occ == 0).sum() >= 50
        assert (np.abs(t - np.ascontiguousarray(d["targets"]["at"][1])) <= np.spacing(np.abs(t))).all()
    at, toward, away = (d["targets"][k][1] for k in ("at", "toward", "away"))
    assert (toward != at).any(axis=1).all() and (away != at).any(axis=1).all()


def test_set_e_direction_scales(orc, sets):
    e = sets("set_e")
    unscaled = e["unscaled"]
    random_exp = sets("bunny")["sets"]["random"][2]
    for name, (o, d, exp, _) in e["trace"].items():
        n = len(o)
        own = np.ones(n, bool)
        if name == "2^-36":
            own[list(qs.THIN_SLOTS)] = False
            assert (np.abs(unscaled[name][~own]).min(axis=1) < 2.0 ** -9).all()
        assert n == 256 and exp[own].tobytes() == random_exp[:n][own].tobytes()
        assert np.array_equal(unscaled[name][own], sets("bunny")["sets"]["random"][1][:n][own])
        x = qs.length2(d)
        assert np.isfinite(x).all() and (x >= np.finfo(F).tiny).all()
        for i in range(n):
            assert qs.unit(orc, d[i]).tobytes() == qs.unit(orc, unscaled[name][i]).tobytes(), (name, i)
        long_way = qs.takes_the_long_way(d)
        groups = long_way[:n - n % 64].reshape(-1, 64).any(axis=1)
        print("E %s: %d rays, %d beyond a gate (%d below the component gate, %d above the length gate); %d of %d whole "
              "groups hold one" % (name, n, long_way.sum(), (np.abs(d).min(axis=1) < qs.COMPONENT_GATE).sum(),
                                   (x > qs.LENGTH2_GATE).sum(), groups.sum(), len(groups)))
        if name == "2^-60":
            assert (np.abs(d).max(axis=1) < qs.COMPONENT_GATE).all()
        elif name == "2^52":
            # (a normal draw shorter than 1/4 stays below the gate; the switch is per wavefront)
            assert (x > qs.LENGTH2_GATE).sum() >= 240 and groups.all()
        elif name == "2^-36":
            assert (np.abs(d).min(axis=1) < qs.COMPONENT_GATE).sum() >= 8 and (~long_way).sum() >= 8
            assert not (x > qs.LENGTH2_GATE).any() and 0 < groups.sum() < len(groups)
        elif name == "2^49":
            assert (x > qs.LENGTH2_GATE).sum() >= 8 and (~long_way).sum() >= 8
            assert not (np.abs(d).min(axis=1) < qs.COMPONENT_GATE).any()
        else:
            assert np.nonzero(long_way)[0].tolist() == list(qs.ONE_LANE_SLOTS) and groups.all()
        assert not qs.takes_the_long_way(unscaled[name]).any()          # unscaled, every ray is on the short way
    for name, (o, t, exp, occ) in e["occlusion"].items():
        v = (t - o).astype(F)
        x = qs.length2(v)
        assert np.isfinite(x).all() and (x >= np.finfo(F).tiny).all()
        long_way = qs.takes_the_long_way(v)
        print("E occlusion %s: %d occluded, %d lit; %d rays beyond a gate" % ((name,) + outcomes(occ) + (long_way.sum(),)))
        assert occ.sum() >= 30 and (occ == 0).sum() >= 30
        # the pair keeps its meaning: fl(target - origin) points along the unscaled direction
        cos = (v.astype(np.float64) * unscaled["2^52"]).sum(axis=1) / np.linalg.norm(v.astype(np.float64), axis=1) \
            / np.linalg.norm(unscaled["2^52"].astype(np.float64), axis=1)
        assert cos.min() > 1.0 - 1e-6
        if name == "2^52":
            assert long_way.sum() >= 240 and long_way.reshape(-1, 64).any(axis=1).all()
        elif name == "2^49":
            assert long_way.sum() >= 8 and (~long_way).sum() >= 8
        else:
            assert np.nonzero(long_way)[0].tolist() == list(qs.ONE_LANE_SLOTS)
