"""The conditions the fixtures of tests/skin_sets.py must meet, asserted without a GPU, with numpy and the oracle alone:
rtx_scene_skinned_prims — the host statement of the skin kernel — word for word against a numpy float32 restatement on
every fixture, the range rule, a -0.0 that `rest` keeps, `one` against the moved pose of the same moves, shared corners
that stay shared, an order of evaluation a reordered or fused kernel cannot reproduce, and the frames each pose changes."""
import importlib

import numpy as np
import pytest

import moves_sets as mv
import prims_sets as pm
import skin_sets as sk
from query_sets import F, bits


@pytest.fixture(scope="module")
def rtx():
    return importlib.import_module("ray-tracer-rust_amd")


@pytest.mark.parametrize("name", sk.POSES)
def test_the_host_statement_is_the_numpy_restatement_word_for_word(rtx, samples_seeded, name):
    y = pm.yard(rtx)
    kw = sk.statement_kw(sk.moves(rtx, name))
    got = sk.stated(rtx, samples_seeded, name)
    want_v, want_s = sk.restated(y["tris"], y["spheres"], **dict(sk.skin(rtx, name), **kw))
    assert np.array_equal(bits(got["tris"]), bits(want_v)), np.argwhere(bits(got["tris"]) != bits(want_v))[:6].tolist()
    assert np.array_equal(bits(got["spheres"]), bits(want_s)), np.argwhere(bits(got["spheres"]) != bits(want_s))[:6].tolist()
    # every posed magnitude is within rtx_scene_pose_bound, and the host variant says so before it looks for a device
    lo, hi = got["spheres"][:, :3] - got["spheres"][:, 3:], got["spheres"][:, :3] + got["spheres"][:, 3:]
    with sk.open_skinned(rtx, samples_seeded, name) as scene:
        bound = scene.pose_bound()
        with pytest.raises(rtx.RtxError) as e:
            scene.pose_skinned(device=99, **sk.moves(rtx, name))
        assert e.value.code == rtx.ERR_NO_DEVICE
    assert np.isfinite(got["tris"]).all() and np.isfinite(got["spheres"]).all()
    assert max(np.abs(got["tris"]).max(), np.abs(lo).max(), np.abs(hi).max()) <= bound == F(10000.0), name
    # the ground stays put: its created values (`one` alone restates them, and loses nothing but the sign of a zero)
    assert np.array_equal(got["tris"][pm.GROUND_NUMBER], y["tris"][pm.GROUND_NUMBER])
    if name != "one":
        assert np.array_equal(bits(got["tris"][pm.GROUND_NUMBER]), bits(y["tris"][pm.GROUND_NUMBER]))


def test_the_host_statement_on_the_count_scenes_and_the_smallest(rtx, samples_seeded):
    for name, sc, skin, kw in sk.count_cases(rtx):
        with pm.open_sized(rtx, samples_seeded, sc) as scene:
            scene.skin(**skin)
            v, s = scene.skinned_prims(**kw)
            bound = scene.pose_bound()
            top = scene.skin_bound()
        want_v, want_s = sk.restated(sc["tris"], sc["spheres"], **dict(skin, **kw))
        assert np.array_equal(bits(v), bits(want_v)) and np.array_equal(bits(s), bits(want_s)), name
        assert (bits(v) != bits(sc["tris"])).any(axis=1).sum() >= len(v) // 2, name          # most of them move
        assert (bits(s) != bits(sc["spheres"])).any(axis=1).sum() >= len(s) // 2, name
        assert max(np.abs(v).max(), np.abs(s[:, :3] - s[:, 3:]).max(), np.abs(s[:, :3] + s[:, 3:]).max()) <= bound, name
        assert top == (True, len(kw["moves"]) - 1), (name, top)
        b = skin["bones"].reshape(-1, 4)
        assert (b == sk.NONE).all(axis=1).any() and ((b == sk.NONE).sum(axis=1) == 1).any(), name      # both kinds of NONE
    assert len(sk.count_cases(rtx)[-1][3]["moves"]) == 257                                    # `many`: 257 moves
    for name, tris, skin, kw in sk.smallest_cases(rtx):
        with sk.open_tris(rtx, samples_seeded, tris) as scene:
            scene.skin(**skin)
            v, s = scene.skinned_prims(**kw)
            assert np.abs(v).max() <= scene.pose_bound(), name
        want_v, _ = sk.restated(tris, np.zeros((0, 4), F), **dict(skin, **kw))
        assert np.array_equal(bits(v), bits(want_v)) and s.shape == (0, 4), name
        assert (bits(v) != bits(tris)).any(axis=1).sum() >= len(v) // 2, name
    assert [3 * len(t) for _, t, _, _ in sk.smallest_cases(rtx)] == [63, 66, 255, 258]


def test_rest_keeps_the_created_words_and_the_sign_of_a_zero(rtx, samples_seeded):
    y = pm.yard(rtx)
    got = sk.stated(rtx, samples_seeded, "rest")
    assert np.array_equal(bits(got["tris"]), bits(y["tris"])) and np.array_equal(bits(got["spheres"]), bits(y["spheres"]))
    assert (np.signbit(sk.ZERO_TRIS[0]) & (sk.ZERO_TRIS[0] == 0)).sum() == 3
    with sk.open_zero(rtx, samples_seeded) as scene:
        bones = np.full((2, 3, 4), sk.NONE, np.uint32)
        scene.skin(bones, np.full((2, 3, 4), 0.25, F))
        kept = scene.skinned_prims(mv.IDENTITY.reshape(1, 12))[0]
        assert np.array_equal(bits(kept), bits(sk.ZERO_TRIS))
        # bones out of range that are not NONE are NONE to the statement
        bones[:] = np.array([1, 2, 0xFFFFFFFE, 65536], np.uint32)
        scene.skin(bones, np.full((2, 3, 4), 0.25, F))
        assert np.array_equal(bits(scene.skinned_prims(mv.IDENTITY.reshape(1, 12))[0]), bits(sk.ZERO_TRIS))
        # ... while the identity matrix in one slot of weight 1 gives the values and not the sign
        bones[:] = sk.NONE
        bones[:, :, 0] = 0
        w = np.zeros((2, 3, 4), F)
        w[:, :, 0] = 1.0
        scene.skin(bones, w)
        unit = scene.skinned_prims(mv.IDENTITY.reshape(1, 12))[0]
        assert np.array_equal(unit, sk.ZERO_TRIS) and not np.signbit(unit).any()


def test_one_is_the_moved_pose_as_values_and_not_in_the_sign_of_a_zero(rtx, samples_seeded):
    kw = sk.statement_kw(sk.moves(rtx, "one"))
    got = sk.stated(rtx, samples_seeded, "one")
    with pm.open_yard(rtx, samples_seeded) as scene:
        v, s = scene.moved_prims(kw["moves"], sk.one_as_groups())
    assert np.array_equal(got["tris"], v) and np.array_equal(got["spheres"], s)               # == : as values
    differs = bits(got["tris"]) != bits(v)
    assert differs.sum() >= 1 and (v[differs] == 0).all() and np.signbit(v[differs]).all() and not np.signbit(got["tris"][differs]).any()


def test_shared_corners_stay_shared_under_bend(rtx, samples_seeded):
    tris, skin = sk.ribbon()
    m = sk.bend_moves(rtx)
    with sk.open_tris(rtx, samples_seeded, tris) as scene:
        scene.skin(**skin)
        v = scene.skinned_prims(m)[0]
    rest, out = bits(tris).reshape(-1, 3), bits(v).reshape(-1, 3)
    pairs = 0
    for a in range(len(rest)):
        for b in range(a + 1, len(rest)):
            if np.array_equal(rest[a], rest[b]):
                pairs += 1
                assert np.array_equal(out[a], out[b]), (a, b)
    assert pairs >= 20 and (out != rest).any(axis=1).sum() >= 40
    # the yard's weights are a function of the rest words too
    h, y = sk.heights(rtx), pm.yard(rtx)["tris"].reshape(-1, 3, 3)
    w = sk.skin(rtx, "bend")["weights"]
    cluster = np.delete(np.arange(len(y)), pm.GROUND_NUMBER)
    assert np.array_equal(w[cluster, :, 1], h[cluster]) and 0.0 == h[cluster].min() and h[cluster].max() == 1.0
    assert len(np.unique(h[cluster])) >= 60


def test_four_cannot_be_reordered_or_fused(rtx, samples_seeded):
    y = pm.yard(rtx)
    kw = sk.statement_kw(sk.moves(rtx, "four"))
    skin = sk.skin(rtx, "four")
    got = sk.stated(rtx, samples_seeded, "four")["tris"]
    assert not np.allclose(skin["weights"].sum(axis=2), 1.0, atol=0.1) and len(np.unique(skin["weights"][0, 0])) == 4
    for form in ("pairwise", "fused"):
        other = sk.restated(y["tris"], y["spheres"], form=form, **dict(skin, **kw))[0]
        assert (bits(other) != bits(got)).sum() >= 1, form
        assert np.allclose(other, got, rtol=1e-5, atol=1e-4), form                  # (the same pose, another rounding)


def test_each_pose_changes_the_frame(rtx, orc, samples_seeded):
    up = pm.posed(orc, rtx, samples_seeded, "identity")["frame"]
    frames = {n: sk.posed(orc, rtx, samples_seeded, n)["frame"] for n in sk.POSES}
    for name in sk.CHANGING:
        assert (frames[name] != up).any(axis=2).sum() >= 20, (name, int((frames[name] != up).any(axis=2).sum()))
    assert (frames["bend"] != frames["one"]).any(axis=2).sum() >= 20
    assert (frames["all"] != frames["bend"]).any(axis=2).sum() >= 20
    assert np.array_equal(frames["rest"], up)
    s = sk.stated(rtx, samples_seeded, "balls")["spheres"]
    assert s[4, 3] == 0 and s[3, 3] == 2 * pm.SPHERES[3, 3] and s[3, 1] - s[3, 3] == 0


def test_no_ray_of_the_views_is_hard_outside_the_hard_ray_set(rtx, orc, samples_seeded):
    for name in ("bend", "all"):
        (ro, rd, exp), (to, tt, texp, occ) = sk.query_set(orc, rtx, samples_seeded, name)
        assert (rd != 0).all() and ((tt - to) != 0).all(), name
        assert 10 <= occ.sum() <= len(occ) - 10, (name, occ.sum())
    ho, hd, exp, twin = sk.hard_rays(orc, rtx, samples_seeded)
    assert (np.signbit(hd) & (hd == 0)).any(axis=1).all()
    k = pm.kinds()
    hit = twin["prim"] != 0xFFFFFFFF
    assert (hit & (k[np.where(hit, twin["prim"], 0)] == 0) & (twin["prim"] != pm.GROUND_AT)).sum() >= 8      # onto the bent cluster
