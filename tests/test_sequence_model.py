"""Is the sequence generator worth running?  CPU only: the model (tests/sequence_model.py), the oracle and the library's
host-only calls.

    restatements    for every drawn moved or skinned pose of every sequence the model's numpy restatement equals
                    rtx_scene_moved_prims / rtx_scene_skinned_prims bit for bit, and rtx_scene_pose_prims_records of the stated
                    arrays equals rtx_scene_posed_records / rtx_scene_rebuilt_records where those apply (spheres and colours
                    as uploaded): the host statements' coverage extended from the yard to the random scenes
    caps            per sequence, with the oracle alone: at most 1/4 of the observations uncompared (the oracle reports a
                    non-finite hit distance: the stress test's cap), at least 3/4 of the state changes SEEN — the expected
                    bytes of the first later observation that depends on the change differ from the expected bytes with the
                    change left out.  An identity move or a recolour of a hidden triangle is allowed only inside that cap:
                    this is what makes a stale flag a failing test rather than an equal frame
    coverage        over the twelve sequences together every transition of the table below occurs
    replays         the same seed gives the same log twice, through RTX_SEQUENCE_SEED / RTX_SEQUENCE_STEPS too

sequence_model.STEPS is the smallest number of steps per sequence, counted up from 40, at which all of this holds."""
import copy
import importlib

import numpy as np
import pytest

import sequence_model as sm
import shade_sets as ss
from query_sets import bits

STRESS_DRAWS = "e13641d15fb82bf359518e764a19d9b8be5fca1e"     # sequence_model.digest of the sixteen draws, made before the move
INDICES = range(len(sm.FAMILY))


@pytest.fixture(scope="module")
def rtx():
    return importlib.import_module("ray-tracer-rust_amd")


@pytest.fixture(scope="module")
def table(samples_seeded):
    return np.ascontiguousarray(samples_seeded[:4096])


_drawn = {}


def drawn(index, table):
    if index not in _drawn:
        _drawn[index] = sm.draw_log(index, table)
    return _drawn[index]


def test_random_scene_moved_unchanged():
    """seed 20261004: the sixteen draws of the stress test, bit for bit"""
    rng = np.random.default_rng(20261004)
    parts = []
    for k in range(16):
        W, H, tris, rgb, spheres, srgb, kinds, kw = sm.random_scene(rng)
        parts += [np.array([W, H]), tris, rgb, spheres, srgb, kinds, np.array(len(repr(sorted(kw.items())).encode())), repr(sorted(kw.items()))]
    assert sm.digest(*parts) == STRESS_DRAWS
    import test_gpu_stress
    assert test_gpu_stress.random_scene is sm.random_scene


@pytest.mark.parametrize("index", INDICES, ids=sm.NAMES)
def test_the_family(rtx, orc, table, index):
    """the pinned counts, the seeds' conditions, and the model's own arithmetic against the library's and the oracle's"""
    spec = sm.FAMILY[index]
    sc = sm.family_scene(spec)
    assert sc["W"] <= 32 and sc["H"] <= 24 and sc["kw"]["nb_light_sample"] in (1, 7, 32) and sc["kw"]["nb_ray"] in (1, 2)
    assert len(sc["tris"]) == spec["n_tris"] + spec["floor"] and len(sc["spheres"]) == spec["n_sph"]
    model = sm.Model(sc, table)
    views = [((sc["W"], sc["H"]), sc["kw"]["eye"], sc["kw"]["look_at"], sc["kw"]["distance"])]
    ex = sm.Expect(orc, sc, views)
    st = ex.frame(model, dict(posed=False, dev=0, view=0))["stats"]
    assert st["primary_hits"] >= 100 and st["nonfinite_t"] == 0, st
    with sm.open_scene(rtx, sc, table) as scene:
        info = scene.info()
        assert scene.pose_bound() == model.bound
        assert info["n_global"] == int(spec["floor"]), info
        if spec["accel"] == sm.ACCEL_BRUTE:
            assert not scene.primary_nodes()[1]                 # it aims nothing
    o, d = sm.ray_arrays(sc["W"], sc["H"], sc["kw"]["eye"], sc["kw"]["look_at"], sc["kw"]["distance"], table, sc["kw"]["nb_ray"])
    ro, rd, _, _, _ = ss.camera_raw_rays(orc, sc["W"], sc["H"], sc["kw"]["eye"], sc["kw"]["look_at"], sm.UP, sc["kw"]["distance"], table,
                                         sc["kw"]["nb_ray"])
    assert np.array_equal(bits(o), bits(ro)) and np.array_equal(bits(d), bits(rd))


def test_the_counts_are_the_kernels_edges():
    assert sorted(f["n_tris"] for f in sm.FAMILY if f["n_tris"]) == [1, 21, 22, 63, 64, 65, 85, 86, 255, 256, 257]
    assert sum(f["n_tris"] == 0 for f in sm.FAMILY) == 1 and len(sm.FAMILY) == 12
    assert {f["floor"] for f in sm.FAMILY} == {False, True} and {f["leaf_max"] for f in sm.FAMILY} == {0, 1, 8}
    assert {f["n_sph"] for f in sm.FAMILY} == {0, 1, 20} and sum(f["accel"] == sm.ACCEL_BRUTE for f in sm.FAMILY) == 1
    assert any(f["n_tris"] == 64 and not f["floor"] and not f["n_sph"] for f in sm.FAMILY)       # 64 primitives, none global


@pytest.mark.parametrize("index", INDICES, ids=sm.NAMES)
def test_restatements_are_the_host_statements(rtx, table, index):
    sc, draw = drawn(index, table)
    model = sm.Model(sc, table)
    checked = 0
    with sm.open_scene(rtx, sc, table) as scene:
        for op in draw.log:
            what = sm.describe(op)
            if op.get("refused"):
                continue
            model.apply(op)
            if op["op"] == "skin":
                scene.skin(op["bones"], op["weights"], op["sphere_bone"])
                assert scene.skin_bound() == (op["bones"] is not None, model.max_bone()), what
            elif op["op"] in ("resample", "reseed"):
                scene.resample(op["table"]) if op["op"] == "resample" else scene.reseed(op["seed"], op["n_pairs"])
                assert np.array_equal(bits(scene.samples_at()), bits(model.table_array())), what
            if op["op"] not in sm.POSE_KINDS:
                continue
            p = model.pose[op["dev"]]
            assert model.in_range(p["tris"], p["spheres"]), what
            if op["op"] == "pose_moved":
                g = op["group"]
                if g is not None and op["variant"] == "device":     # what the device takes as RTX_MOVE_NONE the host variant refuses
                    g = np.where(g >= len(op["moves"]), sm.NONE, g).astype(np.uint32)
                v, s = scene.moved_prims(op["moves"], g, op["radius_scale"])
            elif op["op"] == "pose_skinned":
                v, s = scene.skinned_prims(op["moves"], op["radius_scale"])
            if p["moved"]:
                assert np.array_equal(bits(v), bits(p["tris"])) and np.array_equal(bits(s), bits(p["spheres"])), what
                checked += 1
            if not len(sc["tris"]):
                continue
            as_uploaded = np.array_equal(bits(p["spheres"]), bits(sc["spheres"])) and not sm.coloured(op)
            if as_uploaded:                                         # where posed_records / rebuilt_records apply
                given = dict(v0v1v2=p["tris"], spheres=p["spheres"] if len(p["spheres"]) else None, rgb=p["rgb"],
                             sphere_rgb=p["sphere_rgb"] if len(p["spheres"]) else None)
                if p["rebuilt"]:
                    got, want = scene.pose_prims_records(rebuilt=True, **given), scene.rebuilt_records(p["tris"])
                else:
                    got, want = scene.pose_prims_records(**given), scene.posed_records(p["tris"])
                for a, b in zip(got, want):
                    assert np.array_equal(a, b), what
    assert checked or not any(o["op"] in ("pose_moved", "pose_skinned") and not o.get("refused") for o in draw.log)


def depends(change, model, ob):
    """does the observation read what the change at `change` wrote"""
    kind = change["op"]
    if kind in sm.POSE_KINDS:
        return ob["posed"] and ob["dev"] == change["dev"]
    if kind in ("resample", "reseed"):
        return ob["kind"] not in ("trace_rays", "occluded_rays")
    p = model.pose[ob["dev"]] if ob["posed"] else None             # a bind: through a skinned pose made after it
    return p is not None and p["kind"] == "pose_skinned" and p["since"] > change["step"]


def overwritten(change, op):
    kind = change["op"]
    if kind in sm.POSE_KINDS:
        return op["op"] in sm.POSE_KINDS and op["dev"] == change["dev"]
    if kind in ("resample", "reseed"):
        return op["op"] in ("resample", "reseed")
    return op["op"] == "skin"


def seen(log, ex, models, k):
    """the change at step k: is it seen by the first later observation that depends on it"""
    change = log[k]
    with_it, without = copy.copy(models[k + 1]), copy.copy(models[k])
    with_it.pose, without.pose = list(with_it.pose), list(without.pose)
    for op in log[k + 1:]:
        if op.get("refused"):
            continue
        if overwritten(change, op):
            return False
        for m in (with_it, without):
            m.apply(op)
            if op["op"] in sm.POSE_KINDS and m.pose[op["dev"]] is not None and m.pose[op["dev"]].get("since") is None:
                m.pose[op["dev"]]["since"] = op["step"]
        if op["op"] == "observe" and depends(change, with_it, op):
            if op["posed"] and without.pose[op["dev"]] is None:
                return True                                         # without the change the call is refused
            return ex.observation(with_it, op)["bytes"] != ex.observation(without, op)["bytes"]
    return False


_caps = {}


def caps(orc, table, index):
    if index in _caps:
        return _caps[index]
    sc, draw = drawn(index, table)
    ex = sm.Expect(orc, sc, draw.views)
    model = sm.Model(sc, table)
    models, observed, skipped = [], 0, 0
    for op in draw.log:
        models.append(copy.copy(model))
        models[-1].pose = list(model.pose)
        model.apply(op)
        if op["op"] in sm.POSE_KINDS and not op.get("refused"):
            model.pose[op["dev"]]["since"] = op["step"]
        if op["op"] == "observe" and not op.get("refused"):
            observed += 1
            skipped += ex.observation(model, op)["skip"]
    models.append(model)
    changes = sm.state_changes(draw.log)
    n_seen = sum(seen(draw.log, ex, models, k) for k in changes)
    ex.close()
    _caps[index] = dict(steps=len(draw.log), observed=observed, skipped=skipped, changes=len(changes), seen=n_seen)
    return _caps[index]


@pytest.mark.parametrize("index", INDICES, ids=sm.NAMES)
def test_caps(orc, table, index):
    sc, draw = drawn(index, table)
    c = caps(orc, table, index)
    print("%-14s seed %d: %d steps, %d/%d observations uncompared (%.0f%%), %d/%d state changes seen (%.0f%%)" % (
        sc["name"], draw.seed, c["steps"], c["skipped"], c["observed"], 100.0 * c["skipped"] / c["observed"], c["seen"], c["changes"],
        100.0 * c["seen"] / c["changes"]))
    assert c["steps"] == sm.sequence_steps()
    assert 4 * c["skipped"] <= c["observed"], c
    assert 4 * c["seen"] >= 3 * c["changes"], c


def test_coverage_over_the_twelve_sequences(table):
    total = None
    for index in INDICES:
        c = sm.coverage(drawn(index, table)[1].log)
        total = c if total is None else {k: total[k] | v for k, v in c.items()}
    pairs = {(a, b) for a in sm.POSE_KINDS for b in sm.POSE_KINDS}
    both = {(k, r) for k in ("pose_prims", "pose_moved", "pose_skinned") for r in (False, True)} | {("pose", False), ("pose_rebuilt", True)}
    for k, v in total.items():
        print("%-40s %s" % (k, ("%d of %d" % (len(v), dict(pairs=25, kinds_rebuilt=8, refusals=len(sm.REFUSALS))[k])) if isinstance(v, set) else v))
    assert total["pairs"] == pairs, sorted(pairs - total["pairs"])
    assert total["kinds_rebuilt"] == both, sorted(both - total["kinds_rebuilt"])
    assert total["refusals"] == set(sm.REFUSALS), sorted(set(sm.REFUSALS) - total["refusals"])
    missing = [k for k, v in total.items() if not isinstance(v, set) and not v]
    assert not missing, missing


def test_the_same_seed_gives_the_same_log(table, monkeypatch):
    first = sm.log_text(sm.draw_log(3, table)[1].log)
    assert first == sm.log_text(drawn(3, table)[1].log) and sm.draw_log(3, table)[1].seed == sm.BASE_SEED + 3
    assert sm.log_text(sm.draw_log(3, table, n_devices=2)[1].log) == sm.log_text(sm.draw_log(3, table, n_devices=2)[1].log)
    monkeypatch.setenv("RTX_SEQUENCE_SEED", "77")
    monkeypatch.setenv("RTX_SEQUENCE_STEPS", "55")
    a, b = sm.draw_log(3, table)[1], sm.draw_log(3, table)[1]
    assert a.seed == 77 and len(a.log) == 55 and sm.log_text(a.log) == sm.log_text(b.log) != first
    monkeypatch.delenv("RTX_SEQUENCE_SEED")
    monkeypatch.delenv("RTX_SEQUENCE_STEPS")
    assert sm.log_text(sm.draw_log(3, table, seed=77, steps=55)[1].log) == sm.log_text(a.log)
    assert {d for op in sm.draw_log(3, table, n_devices=2)[1].log for d in [op.get("dev", 0)]} == {0, 1}
