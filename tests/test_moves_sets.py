"""The conditions the fixtures of tests/moves_sets.py must meet, asserted without a GPU: rtx_scene_moved_prims — the host
statement of the move kernel — word for word against a numpy float32 restatement on every fixture, the range rule, the
frames each pose changes (the oracle alone), RTX_MOVE_NONE against the identity matrix, and the rays of the fixtures'
views."""
import importlib

import numpy as np
import pytest

import moves_sets as mv
import prims_sets as pm
from query_sets import F, bits


@pytest.fixture(scope="module")
def rtx():
    return importlib.import_module("ray-tracer-rust_amd")


@pytest.mark.parametrize("name", mv.POSES)
def test_the_host_statement_is_the_numpy_restatement_word_for_word(rtx, samples_seeded, name):
    y = pm.yard(rtx)
    kw = mv.statement_kw(mv.moves(rtx, name))
    got = mv.stated(rtx, samples_seeded, name)
    want_v, want_s = mv.restated(y["tris"], y["spheres"], y["kinds"], **kw)
    assert np.array_equal(bits(got["tris"]), bits(want_v)), np.argwhere(bits(got["tris"]) != bits(want_v))[:6].tolist()
    assert np.array_equal(bits(got["spheres"]), bits(want_s)), np.argwhere(bits(got["spheres"]) != bits(want_s))[:6].tolist()
    # every posed magnitude is within rtx_scene_pose_bound
    lo, hi = got["spheres"][:, :3] - got["spheres"][:, 3:], got["spheres"][:, :3] + got["spheres"][:, 3:]
    with pm.open_yard(rtx, samples_seeded) as scene:
        bound = scene.pose_bound()
    assert np.isfinite(got["tris"]).all() and np.isfinite(got["spheres"]).all()
    assert max(np.abs(got["tris"]).max(), np.abs(lo).max(), np.abs(hi).max()) <= bound == F(10000.0), name
    # the ground and whatever follows no move: the created words
    assert np.array_equal(bits(got["tris"][pm.GROUND_NUMBER]), bits(y["tris"][pm.GROUND_NUMBER]))


def test_the_host_statement_on_the_count_scenes(rtx, samples_seeded):
    for name, sc, kw in mv.count_cases(rtx):
        with pm.open_sized(rtx, samples_seeded, sc) as scene:
            v, s = scene.moved_prims(**kw)
            bound = scene.pose_bound()
        want_v, want_s = mv.restated(sc["tris"], sc["spheres"], sc["kinds"], **kw)
        assert np.array_equal(bits(v), bits(want_v)) and np.array_equal(bits(s), bits(want_s)), name
        assert (bits(v) != bits(sc["tris"])).any(axis=1).sum() >= len(v) // 2, name          # most of them move
        assert (bits(s) != bits(sc["spheres"])).any(axis=1).sum() >= len(s) // 2, name
        assert max(np.abs(v).max(), np.abs(s[:, :3] - s[:, 3:]).max(), np.abs(s[:, :3] + s[:, 3:]).max()) <= bound, name
    assert len(mv.count_cases(rtx)[-1][2]["moves"]) == 257                                    # `many`: a move per primitive


def test_each_pose_changes_the_frame(rtx, orc, samples_seeded):
    up = pm.posed(orc, rtx, samples_seeded, "identity")["frame"]
    frames = {n: mv.posed(orc, rtx, samples_seeded, n)["frame"] for n in mv.POSES}
    for name in mv.CHANGING:
        assert (frames[name] != up).any(axis=2).sum() >= 20, (name, int((frames[name] != up).any(axis=2).sum()))
    assert (frames["all"] != frames["turn"]).any(axis=2).sum() >= 20
    assert np.array_equal(frames["same"], up) and np.array_equal(frames["unit"], up)
    # shear: neighbouring triangles of the cluster follow different moves
    g = mv.moves(rtx, "shear")["group"][mv.cluster_at()]
    assert (g[1:] != g[:-1]).sum() >= 10 and set(g) == {0, 1}
    # balls: a radius of 0 and a doubled one that still touches the ground
    s = mv.stated(rtx, samples_seeded, "balls")["spheres"]
    assert s[4, 3] == 0 and s[3, 3] == 2 * pm.SPHERES[3, 3] and s[3, 1] - s[3, 3] == 0


def test_none_and_the_identity_matrix_give_the_created_words(rtx, samples_seeded):
    y = pm.yard(rtx)
    assert not (np.signbit(y["tris"]) & (y["tris"] == 0)).any() and not (np.signbit(y["spheres"]) & (y["spheres"] == 0)).any(), \
        "the yard holds a -0.0 coordinate: the identity matrix would not keep it"
    for name in ("same", "unit"):
        got = mv.stated(rtx, samples_seeded, name)
        assert np.array_equal(bits(got["tris"]), bits(y["tris"])) and np.array_equal(bits(got["spheres"]), bits(y["spheres"])), name
    # ... and where there is one, RTX_MOVE_NONE keeps its sign and the identity matrix does not
    tri = np.array([[-0.0, 1, 2, 3, -0.0, 5, 6, 7, -0.0]], F)
    with rtx.Scene(8, 8, tri, np.ones((1, 3), F), samples_seeded[:4096], nb_light_sample=4, reference_tree=rtx.REFTREE_NEVER,
                   tie_rank=None) as scene:
        kept = scene.moved_prims(mv.IDENTITY.reshape(1, 12), np.array([mv.NONE], np.uint32))[0]
        unit = scene.moved_prims(mv.IDENTITY.reshape(1, 12))[0]
    assert np.array_equal(bits(kept), bits(tri))
    assert np.array_equal(unit, tri) and not np.signbit(unit).any()


def test_no_ray_of_the_views_is_hard_outside_the_hard_ray_set(rtx, orc, samples_seeded):
    o, d = mv.view_rays(orc, samples_seeded)
    assert (d != 0).all()
    for name in ("turn", "all"):
        (ro, rd, exp), (to, tt, texp, occ) = mv.query_set(orc, rtx, samples_seeded, name)
        assert (rd != 0).all() and ((tt - to) != 0).all(), name
        assert 10 <= occ.sum() <= len(occ) - 10, (name, occ.sum())
    ho, hd, exp, twin = mv.hard_rays(orc, rtx, samples_seeded)
    assert (np.signbit(hd) & (hd == 0)).any(axis=1).all()
    assert (exp["prim"] != twin["prim"]).sum() >= 8                               # the oracle's own tree walks past some
    k = pm.kinds()
    hit = twin["prim"] != 0xFFFFFFFF
    assert (hit & (k[np.where(hit, twin["prim"], 0)] == 0) & (twin["prim"] != pm.GROUND_AT)).sum() >= 8      # onto the turned cluster
