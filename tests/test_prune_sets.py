"""The conditions the fixtures of tests/prune_sets.py must meet to test what they are for — the distance pruning of the
closest-hit walks against triangles whose computed distance is far from where they lie — checked with the CPU oracle and
the library's host-side scene read-back alone.  They are conditions on the inputs: a fixture that misses one gets another
seed, not a lower threshold.  Each assertion's message states the counts (pytest -s prints them as well)."""
import importlib

import numpy as np
import pytest

import prune_sets as ps
from query_sets import NO_HIT

NAMES = ("triangles", "sphere")


@pytest.fixture(scope="module")
def rtx():
    return importlib.import_module("ray-tracer-rust_amd")


@pytest.fixture(scope="module")
def fx(rtx, orc, samples_seeded):
    class Fixtures:
        scene = staticmethod(lambda name: ps.scene(rtx, orc, samples_seeded, name))
        rays = staticmethod(lambda name: ps.ray_sets(rtx, orc, samples_seeded, name))
        checked = staticmethod(lambda name, order, key, wave=1: ps.checked(rtx, orc, samples_seeded, name, order, key, wave))
    return Fixtures


@pytest.mark.parametrize("name", NAMES)
def test_the_wall_and_the_triangles_behind_it_sit_in_different_leaves(fx, name):
    for order, b in fx.scene(name).items():
        LEAF = ps.LEAF
        assert b.info["n_global"] == 0 and b.info["max_leaf_tris"] <= 4, b.info
        # the stream says the same: record 1 is not a leaf of global triangles under an untested root (walk_stream)
        leaves = np.nonzero(b.nodes[:, 7] & LEAF)[0]
        assert (b.nodes[leaves, 3] <= 4).all() and int(b.nodes[leaves, 3].sum()) == b.n
        assert not b.nodes[0, 7] & LEAF and int(b.nodes[0, 3]) == len(b.nodes)
        wall, behind = set(b.leaf_of[b.groups["wall"]].tolist()), set(b.leaf_of[b.groups["behind"]].tolist())
        assert len(b.groups["wall"]) >= 8 and not wall & behind, (order, wall, behind)
        assert not wall & set(b.leaf_of[b.groups["front"]].tolist())
        if name == "triangles":
            assert np.array_equal(np.argsort(b.rank), np.argsort(b.ref_rank))      # the oracle's leaf order is rtxh_ref_leaf_rank's
        # the two orders walk the wall and the group behind it in opposite orders
    a, m = fx.scene(name)["built"], fx.scene(name)["mirrored"]
    first = lambda b, g: int(b.leaf_of[b.groups[g]].min())
    assert first(a, "wall") < first(a, "behind") and first(m, "behind") < first(m, "wall")


@pytest.mark.parametrize("name", NAMES)
def test_at_least_128_rays_of_one_triangle_are_exposed(fx, name):
    r = fx.rays(name)
    print("%s: %d of %d drawn rays picked by np_ref; exposed by the emulation: %s; batches from '%s'"
          % (name, r["likely"], ps.N_DRAWS, r["counts"], r["chosen_order"]))
    assert r["chosen_order"] is not None, "no order exposes %d rays: %s" % (ps.N_EXPOSED, r["counts"])
    order, target = r["chosen_order"], r["exposed_prim"]
    b = fx.scene(name)[order]
    assert target in b.groups["behind"]
    o, d, exp, units = r[order]["exposed"]
    assert len(o) == ps.N_EXPOSED and (exp["prim"] == target).all()
    wall_t = np.abs(ps.WALL_Z / units[:, 2].astype(np.float64))
    # the oracle's distance lies in front of the wall although the triangle's own box begins behind it
    entry = np.array([ps.box_entry(b.lo[target], b.hi[target], np.zeros(3), u.astype(np.float64), 0.0)[1] for u in units])
    assert (exp["t"] < wall_t).all() and (entry > wall_t * (1.0 + 2.0 ** -15)).all()
    print("%s: t of the triangle behind %.2f .. %.2f, the wall at %.2f .. %.2f, entry into the triangle's box %.2f .. %.2f"
          % (name, exp["t"].min(), exp["t"].max(), wall_t.min(), wall_t.max(), entry.min(), entry.max()))
    for wave in (1, 64):                    # alone (a), and as two whole wavefronts in the caller's order (b)
        agrees, exposed = fx.checked(name, order, "exposed", wave)
        assert agrees.all() and exposed.sum() == ps.N_EXPOSED, \
            "%s %s, %d rays to a wavefront: %d of %d exposed" % (name, order, wave, exposed.sum(), ps.N_EXPOSED)
    # every walking lane takes the multiply-based test: regular directions (closest_hit), origins inside the bound
    assert (np.abs(units) >= 2.0 ** -60).all() and (np.abs(units) <= 2.0).all() and not o.any()


@pytest.mark.parametrize("name", NAMES)
def test_the_unpruned_emulation_is_the_oracle_on_every_ray(fx, name):
    r = fx.rays(name)
    for order in ps.ORDERS:
        sets = r[order]
        n = len(sets["ordinary"][0])
        assert n == 1000 and len(sets["mixed"][0]) == n + ps.N_EXPOSED
        # `mixed` is the exposed rays at r['place'] among the ordinary ones, record for record
        rest = np.setdiff1d(np.arange(n + ps.N_EXPOSED), r["place"])
        for k in range(4):
            assert np.array_equal(sets["mixed"][k][r["place"]], sets["exposed"][k]) and np.array_equal(sets["mixed"][k][rest], sets["ordinary"][k])
        counts = {}
        for key in sets:
            if key == "mixed":
                agrees, exposed = fx.checked(name, order, key, 64)          # default flags: 64 consecutive rays to a wavefront
            else:
                agrees, exposed = fx.checked(name, order, key)
            counts[key] = int(exposed.sum())
            assert agrees.all(), "%s %s %s: the unpruned emulation differs from the oracle at %s" % (name, order, key, np.nonzero(~agrees)[0][:8])
        print("%s %s: exposed rays per set %s" % (name, order, counts))
        for key in set(sets) - {"exposed", "mixed"}:
            assert counts[key] == 0, "%s %s: %d exposed rays among the controls '%s'" % (name, order, counts[key], key)
        hit = sets["ordinary"][2]["prim"] != NO_HIT
        assert hit.sum() >= 500 and (~hit).sum() >= 50 and np.isin(sets["ordinary"][2]["prim"][hit], fx.scene(name)[order].groups["wall"]).all()


@pytest.mark.parametrize("name", NAMES)
def test_the_controls_show_both_outcomes(orc, fx, name):
    r = fx.rays(name)
    for order in ps.ORDERS:
        b, sets = fx.scene(name)[order], r[order]
        wall = b.groups["wall"]
        # a triangle in FRONT of the wall: it wins where its distance comes out in front, and loses where it comes out behind
        o, _, exp, units = sets["front"]
        behind = wins = 0
        for k in range(len(o)):
            cand = ps.candidates(orc, b, o[k], units[k])
            front = [cand[p] for p in b.groups["front"] if p in cand]
            if exp["prim"][k] in b.groups["front"]:
                wins += 1
            elif front and exp["prim"][k] in wall and min(front) > exp["t"][k]:
                behind += 1
        print("%s %s: a triangle in front of the wall wins %d rays and is computed behind it in %d" % (name, order, wins, behind))
        assert wins >= 16 and behind >= 4, (name, order, wins, behind)
        # well-conditioned triangles and the sphere behind the wall are met (a candidate exists) and lose to the wall
        for key in ("well", "sphere") if name == "sphere" else ("well",):
            o, _, exp, units = sets[key]
            met = sum(1 for k in range(len(o)) if any(p in ps.candidates(orc, b, o[k], units[k]) for p in b.groups[key]))
            print("%s %s: %d of %d rays meet '%s' behind the wall" % (name, order, met, len(o), key))
            assert np.isin(exp["prim"], wall).all() and met >= 48, (name, order, key, met)


@pytest.mark.parametrize("name", NAMES)
def test_the_shaded_batch_tells_the_two_answers_apart(orc, samples_seeded, fx, name):
    """rtx_shade_rays on the exposed rays: the colours of the oracle's answer against those of a scene without the
    triangle (the wall's points), and the composition against the oracle's own render_pixel is tests/test_shade_sets.py's"""
    r = fx.rays(name)
    order = r["chosen_order"]
    b = fx.scene(name)[order]
    s = ps.shade_batch(orc, b, samples_seeded, r[order]["exposed"])
    wrong = ps.shade_batch(orc, b, samples_seeded, r[order]["exposed"], osc=ps.without(orc, b, r["exposed_prim"]))
    differ = int((s["shade"]["rgb8"] != wrong["shade"]["rgb8"]).any(axis=1).sum())
    print("%s %s: %d of %d shaded rays differ in RGB8 from the scene without the triangle" % (name, order, differ, ps.N_EXPOSED))
    assert np.array_equal(s["hit"]["prim"], r[order]["exposed"][2]["prim"]) and differ >= 64, differ


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("order", ps.ORDERS)
def test_the_one_ray_of_the_frame_is_exposed(rtx, orc, samples_half, fx, name, order):
    f = ps.frame(rtx, orc, samples_half, name, order)
    assert f["exposed"], "%s %s: none of %d rays through a frame's centre is exposed" % (name, order, f["tried"])
    b, (o, d) = f["b"], f["ray"]
    print("%s %s: look_at %s, point %d of the draw; the oracle answers primitive %d at t = %.3f"
          % (name, order, f["camera"]["look_at"], f["tried"], f["exp"]["prim"][0], f["exp"]["t"][0]))
    assert (b.args[0], b.args[1]) == (1, 1) and f["exp"]["prim"][0] == f["target"] and not o.any()
    assert b.info["n_global"] == 0 and (np.abs(d) >= 2.0 ** -60).all()
    # the frame's pixel is that ray's: the oracle scene of this camera hits the same primitive
    _, st, tri = b.osc.render_rows(mode=orc.MODE_BVH, want_tri=True)
    assert tri.shape == (1, 1) and tri[0, 0] == f["target"] and st["primary_hits"] == 1
    # the pixel's bytes tell the two answers apart: lit, and not what the scene gives with that triangle taken away
    print("%s %s: the pixel is %s, without the triangle %s" % (name, order, f["ref"][0, 0].tolist(), f["without"][0, 0].tolist()))
    assert f["ref"].any() and f["without"].any() and not np.array_equal(f["ref"], f["without"])
    # the emulation walked the primary rays' own stream (the child nearer the eye first): the wall before what lies behind it
    assert b.primary_own and len(b.primary) == len(b.nodes)
    # rtx_render_view walks the library's own stream: there the same ray is exposed in the order that exposes the ray sets
    print("%s %s: on the own stream of the ray sets' scene the ray is %sexposed" % (name, order, "" if f["exposed_on_nodes"] else "not "))
    assert np.array_equal(f["seen"].nodes, fx.scene(name)[order].nodes)
    assert f["exposed_on_nodes"] == (order == fx.rays(name)["chosen_order"]), (name, order)
