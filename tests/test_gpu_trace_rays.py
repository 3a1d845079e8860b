"""GPU parity of the ray-query entry points (rtx_trace_rays, rtx_occluded_rays, and their device-resident variants)
against the CPU oracle's orc_closest_hit, one caller-supplied ray at a time: primitive, and the bit patterns of t and
p_hit; a triangle's normal is the scene's stored normal, a sphere's a float32 restatement of sphere.rs:93-95.  Every
ray set is traced in the caller's order, in the default mode and with the regrouping pass forced (the sets are smaller
than the library's threshold), with and without statistics: all must be the same bytes."""
import importlib
import os

import numpy as np
import pytest

import np_ref
from query_sets import (F, H, LIGHT_POINT, NO_HIT, W, bits, bunny_random_sets, check_hits, expected_occlusion,
                        oracle_hits)
from test_gpu_spheres import KAT, kat_scene

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def rtx():
    mod = importlib.import_module("ray-tracer-rust_amd")
    assert mod.device_count() >= 1, "no HIP device: the product path has no CPU fallback"
    return mod


def primaries(orc, eye, look_at, up, distance, samples, scale=1.0):
    """the W x H primary rays (sample 0) of a camera by orc_create_ray, directions multiplied by `scale`"""
    L = orc.lib()
    u, v, w = (np.zeros(3, F) for _ in range(3))
    L.orc_camera_new(orc._fp(orc.f3(eye)), orc._fp(orc.f3(look_at)), orc._fp(orc.f3(up)), orc._fp(u), orc._fp(v), orc._fp(w))
    o, d = np.zeros((W * H, 3), F), np.zeros((W * H, 3), F)
    e = orc.f3(eye)
    for py in range(H):
        for px in range(W):
            k = py * W + px
            L.orc_create_ray(px, py, 0, W, H, orc._fp(e), orc._fp(u), orc._fp(v), orc._fp(w), float(distance),
                             orc._fp(samples), len(samples), orc._fp(o[k]), orc._fp(d[k]))
    return o, (d * F(scale)).astype(F)


def trace_every_way(scene, o, d, exp, normals, what):
    """caller's order, default, forced regrouping x with / without statistics: the oracle's answer, the same bytes"""
    first = None
    for mode in (dict(keep_order=True), dict(), dict(force_regroup=True)):
        for stats in (False, True):
            got = scene.trace_rays(o, d, stats=stats, **mode)
            if stats:
                got, st = got
                assert st["primary_hits"] == int((exp["prim"] != NO_HIT).sum()), (what, mode)
                assert st["primary_rays"] == st["rays"] == len(o) and st["shadow_rays"] == 0
            check_hits(got, exp, normals, "%s %s stats=%s" % (what, mode, stats))
            first = got if first is None else first
            assert got.tobytes() == first.tobytes(), "%s: %s stats=%s differs from the first call" % (what, mode, stats)
    return first


def occluded_every_way(scene, o, t, want, what):
    for mode in (dict(keep_order=True), dict(), dict(force_regroup=True)):
        for stats in (False, True):
            got = scene.occluded_rays(o, t, stats=stats, **mode)
            if stats:
                got, st = got
                assert st["primary_hits"] == int(want.sum()) and st["rays"] == len(o) and st["shadow_rays"] == 0
            assert np.array_equal(got, want), "%s %s stats=%s: %d rays differ" % (what, mode, stats, int((got != want).sum()))


@pytest.fixture(scope="module")
def bunny(rtx, orc, samples_seeded):
    """big_bunny + ground (4,969 primitives, reference tree built), and the ray sets with the oracle's answers"""
    osc = orc.default_scene(["big_bunny.obj"], W, H, samples_seeded)
    scene = rtx.default_scene([os.path.join(ROOT, "models", "big_bunny.obj")], W, H, samples_seeded)
    assert scene.info()["n_tris"] == 4969 and scene.info()["n_ref_nodes"] != 0
    dt = rtx.rtx.RAY_HIT_DTYPE
    sets = {}
    o, d = primaries(orc, orc.EYE, orc.LOOK_AT, orc.UP, orc.DISTANCE, samples_seeded, scale=3.5)
    sets["primary"] = (o, d) + oracle_hits(orc, osc, o, d, dt)
    lo = sets["primary"][2]["p_hit"].copy()
    ld = (np.asarray(LIGHT_POINT, F) - lo).astype(F)
    sets["to_light"] = (lo, ld) + oracle_hits(orc, osc, lo, ld, dt)
    sets.update(bunny_random_sets(orc, osc, dt))       # "random" and "random_targets"
    yield dict(scene=scene, osc=osc, sets=sets, normals=scene.normals(), ground=len(scene.tris) - 1)
    scene.close()
    osc.close()


def test_primary_like_rays_with_unnormalised_directions(bunny):
    o, d, exp, _ = bunny["sets"]["primary"]
    assert int((exp["prim"] != NO_HIT).sum()) >= 1000
    assert not np.allclose(np.linalg.norm(d, axis=1), 1.0, atol=0.5)          # the library normalises, not the caller
    trace_every_way(bunny["scene"], o, d, exp, bunny["normals"], "primary-like")


def test_rays_from_the_hit_points_to_the_light(bunny):
    o, d, exp, _ = bunny["sets"]["to_light"]
    hits = int((exp["prim"] != NO_HIT).sum())
    assert hits >= 200 and len(o) - hits >= 400
    trace_every_way(bunny["scene"], o, d, exp, bunny["normals"], "to-light")


def test_random_rays(bunny):
    o, d, exp, _ = bunny["sets"]["random"]
    hit = exp["prim"] != NO_HIT
    assert hit.sum() >= 500 and (hit & (exp["prim"] != bunny["ground"])).sum() >= 100 and (~hit).sum() >= 400
    assert np.isfinite(exp["t"]).all()
    trace_every_way(bunny["scene"], o, d, exp, bunny["normals"], "random")


@pytest.mark.parametrize("n", [1, 63, 64, 65])
def test_batch_sizes_around_one_wavefront(bunny, n):
    """prefixes of the random set: a lone ray, one lane short of a wavefront, exactly one, one lane into the second"""
    o, d, exp, _ = bunny["sets"]["random"]
    trace_every_way(bunny["scene"], o[:n], d[:n], exp[:n], bunny["normals"], "random[:%d]" % n)


@pytest.mark.parametrize("dx,groups", [(-0.0, 1), (0.0, 0)])
def test_a_hard_ray_sends_its_group_through_the_reference_walk(rtx, orc, bunny, dx, groups):
    """From (-20, 200, 0) straight down: with d.x = -0.0 the reference's own tree rejects at an ancestor box what the leaf
    would accept (a miss), with d.x = +0.0 the ray hits primitive 3591.  The -0.0 ray is "hard": its 64-ray group is traced
    whole by the literal reference walk, and the 63 regular rays beside it keep the oracle's answers."""
    o, d, exp, _ = bunny["sets"]["random"]
    o = np.concatenate([o[:63], np.array([[-20.0, 200.0, 0.0]], F)])
    d = np.concatenate([d[:63], np.array([[dx, -1.0, 0.0]], F)])
    assert np.signbit(d[63, 0]) == (groups == 1)
    own, _ = oracle_hits(orc, bunny["osc"], o[63:], d[63:], rtx.rtx.RAY_HIT_DTYPE)
    if groups:
        assert own["prim"][0] == NO_HIT
    else:
        assert own["prim"][0] == 3591 and abs(float(own["t"][0]) - 76.6837) < 1e-3
    exp = np.concatenate([exp[:63], own])
    trace_every_way(bunny["scene"], o, d, exp, bunny["normals"], "hard ray dx=%r" % dx)
    for mode in (dict(keep_order=True), dict(force_regroup=True)):
        _, st = bunny["scene"].trace_rays(o, d, stats=True, **mode)
        assert st["redo_tiles"] == groups, (mode, st["redo_tiles"])
    # the occlusion call in such a group: main.rs:220 on that walk's closest hit.  target - origin keeps a -0.0 only as
    # (-0.0) - (+0.0), so this ray starts at x = +0.0
    oo = o.copy()
    oo[63] = (0.0, 200.0, 0.0)
    t = (oo + d * F(50.0)).astype(F)
    t[63] = (dx, 100.0, 0.0)
    v = (t - oo).astype(F)
    assert np.signbit(v[63, 0]) == (groups == 1)
    texp, _ = oracle_hits(orc, bunny["osc"], oo, v, rtx.rtx.RAY_HIT_DTYPE)
    want = expected_occlusion(texp, oo, t)
    assert 0 < want.sum() < 64
    occluded_every_way(bunny["scene"], oo, t, want, "occlusion beside dx=%r" % dx)
    _, st = bunny["scene"].occluded_rays(oo, t, stats=True, keep_order=True)
    assert st["redo_tiles"] == groups


def test_exact_tie_and_hits_closer_than_one(rtx, orc, samples_seeded):
    """Coincident triangles: every hit is an exact distance tie and the right-most leaf of the reference's tree wins
    (bvh.rs:123-130).  A triangle nearer than t = 1.0 is invisible, the one behind it is hit (bvh.rs:64-67)."""
    cam = dict(eye=(0.0, 0.0, 0.0), look_at=(0.0, 0.0, -1.0), up=(0.0, 1.0, 0.0), distance=16.0,
               light_tri=(-1.0, 50.0, -1.0, 1.0, 50.0, -1.0, 0.0, 50.0, 1.0))
    o, d = primaries(orc, cam["eye"], cam["look_at"], cam["up"], cam["distance"], samples_seeded)
    big = [-30.0, -30.0, -20.0, 30.0, -30.0, -20.0, 0.0, 30.0, -20.0]
    near = [-3.0, -3.0, -0.5, 3.0, -3.0, -0.5, 0.0, 3.0, -0.5]
    for what, tris, only in (("tie", [big] * 5, None), ("t < 1", [near, big], 1)):
        tris = np.array(tris, F)
        rgb = np.ones((len(tris), 3), F)
        osc = orc.Scene(W, H, tris, rgb, samples_seeded, **cam)
        exp, _ = oracle_hits(orc, osc, o, d, rtx.rtx.RAY_HIT_DTYPE)
        hit = exp["prim"] != NO_HIT
        assert hit.sum() > 100
        winner = int(osc.leaf_order()[-1]) if only is None else only
        assert (exp["prim"][hit] == winner).all()
        with rtx.Scene(W, H, tris, rgb, samples_seeded, **cam) as s:
            trace_every_way(s, o, d, exp, s.normals(), what)
        osc.close()


def test_spheres(rtx, orc, samples_seeded):
    """kat_scene of tests/test_gpu_spheres.py, interleaved kinds: hits on spheres 1 and 2, none on 4 (around the eye: t < 1)."""
    tris, rgb, spheres, srgb, kinds = kat_scene()
    o, d = primaries(orc, KAT["eye"], KAT["look_at"], KAT["up"], KAT["distance"], samples_seeded)
    osc = orc.Scene(W, H, tris, rgb, samples_seeded, spheres=spheres, sphere_rgb=srgb, kinds=kinds, **KAT)
    exp, _ = oracle_hits(orc, osc, o, d, rtx.rtx.RAY_HIT_DTYPE)
    assert (exp["prim"] == 1).sum() > 10 and (exp["prim"] == 2).sum() > 10 and (exp["prim"] == 4).sum() == 0
    with rtx.Scene(W, H, tris, rgb, samples_seeded, spheres=spheres, sphere_rgb=srgb, kinds=kinds, **KAT) as s:
        stored = s.normals()
        got = trace_every_way(s, o, d, exp, None, "spheres")
    with rtx.Scene(W, H, tris, rgb, samples_seeded, spheres=spheres, sphere_rgb=srgb, kinds=kinds, accel=1, **KAT) as brute:
        assert brute.trace_rays(o, d).tobytes() == got.tobytes()
    is_sphere = np.zeros(len(exp), bool)
    hit = exp["prim"] != NO_HIT
    is_sphere[hit] = kinds[exp["prim"][hit]] == 1
    assert np.array_equal(bits(got["normal"][hit & ~is_sphere]), bits(stored[exp["prim"][hit & ~is_sphere]]))
    p = got["p_hit"][is_sphere]
    want = np.stack(np_ref._normalize(np_ref._sub(np_ref._v(p), np_ref._v(stored[exp["prim"][is_sphere]]))), axis=-1)   # sphere.rs:93-95
    assert np.array_equal(bits(got["normal"][is_sphere]), bits(want))
    osc.close()


@pytest.mark.parametrize("kw", [dict(accel=1), dict(reference_tree=2)], ids=["brute", "no_reference_tree"])
def test_other_build_options_give_the_same_bytes(rtx, bunny, samples_seeded, kw):
    """accel = RTX_ACCEL_BRUTE and reference_tree = RTX_REFTREE_NEVER on the random set (regular rays only; the oracle
    counts no exact tie on it: the result does not depend on the tree)"""
    o, d, exp, _ = bunny["sets"]["random"]
    want = bunny["scene"].trace_rays(o, d, keep_order=True)
    ro, targets, _, _ = bunny["sets"]["random_targets"]
    want_occ = bunny["scene"].occluded_rays(ro, targets, keep_order=True)
    with rtx.default_scene([os.path.join(ROOT, "models", "big_bunny.obj")], W, H, samples_seeded, **kw) as s:
        if "reference_tree" in kw:
            assert s.info()["n_ref_nodes"] == 0
        for mode in (dict(keep_order=True), dict(force_regroup=True)):
            assert s.trace_rays(o, d, **mode).tobytes() == want.tobytes(), mode
            assert np.array_equal(s.occluded_rays(ro, targets, **mode), want_occ), mode
    check_hits(want, exp, bunny["normals"], "random")


def test_occlusion(bunny):
    """the to-light set (origins = the primary hit points, target = a light point) and random point pairs"""
    lo, _, lexp, _ = bunny["sets"]["to_light"]
    lt = np.tile(np.asarray(LIGHT_POINT, F), (len(lo), 1))
    want = expected_occlusion(lexp, lo, lt)
    assert want.sum() >= 100 and (want == 0).sum() >= 100
    occluded_every_way(bunny["scene"], lo, lt, want, "to-light")
    ro, targets, rexp, _ = bunny["sets"]["random_targets"]
    want = expected_occlusion(rexp, ro, targets)
    assert want.sum() >= 100 and (want == 0).sum() >= 100
    occluded_every_way(bunny["scene"], ro, targets, want, "random pairs")
    for n in (1, 63, 64, 65):
        occluded_every_way(bunny["scene"], ro[:n], targets[:n], want[:n], "random pairs[:%d]" % n)


def test_device_resident_calls_on_a_stream_of_their_own(rtx, orc, bunny, samples_seeded):
    torch = pytest.importorskip("torch")
    assert torch.cuda.is_available(), "torch sees no GPU"
    scene = bunny["scene"]
    o, d, _, _ = bunny["sets"]["random"]
    _, targets, _, _ = bunny["sets"]["random_targets"]
    host_hits = scene.trace_rays(o, d)
    host_occ = scene.occluded_rays(o, targets)
    n = len(o)
    stream = torch.cuda.Stream(device="cuda:0")
    assert stream.cuda_stream != torch.cuda.default_stream().cuda_stream
    with torch.cuda.stream(stream):
        t_o = torch.from_numpy(o).to("cuda:0")
        t_d = torch.from_numpy(d).to("cuda:0")
        t_t = torch.from_numpy(targets).to("cuda:0")
        hits = torch.full((n * 32,), 0xAA, dtype=torch.uint8, device="cuda:0")
        occ = torch.full((n,), 0xAA, dtype=torch.uint8, device="cuda:0")
        for mode in (dict(keep_order=True), dict(force_regroup=True)):
            scene.trace_rays_device(0, n, t_o.data_ptr(), t_d.data_ptr(), hits.data_ptr(), stream.cuda_stream, **mode)
            scene.occluded_rays_device(0, n, t_o.data_ptr(), t_t.data_ptr(), occ.data_ptr(), stream.cuda_stream, **mode)
            stream.synchronize()
            assert hits.cpu().numpy().tobytes() == host_hits.tobytes(), mode
            assert np.array_equal(occ.cpu().numpy(), host_occ), mode
            hits.fill_(0xAA)
            occ.fill_(0xAA)
        stream.synchronize()
    # a query leaves the render workspace alone: the frame is still the oracle's
    img = scene.render_rows()
    ref, _ = bunny["osc"].render_rows(mode=orc.MODE_BVH)
    assert np.array_equal(img, ref)


@pytest.mark.parametrize("scale", [10, 100, 1000])
def test_origins_far_outside_the_scene(rtx, orc, bunny, scale):
    """Origins at 10, 100 and 1000 times the scene's extent (the ground reaches +-10,000), aimed at points inside the mesh's
    box: a pick ray from a distant camera.  The multiply-based culling of the walk is proven for origins no farther out
    than the scene's own coordinates; a group holding a farther one must walk with the exact box test and give the
    oracle's answer.  A mixed batch — far rays interleaved with the random set's — must too, in every order."""
    rng = np.random.default_rng(11 + scale)
    u = rng.normal(size=(200, 3))
    u /= np.linalg.norm(u, axis=1)[:, None]
    o = (u * scale * 1e4).astype(F)
    target = rng.uniform((-90.0, 35.0, -60.0), (60.0, 180.0, 55.0), size=(200, 3)).astype(F)
    d = (target - o).astype(F)
    assert np.abs(o).max(axis=1).min() > 10000.0 * scale / 2.0             # every origin is beyond the proven range
    exp, _ = oracle_hits(orc, bunny["osc"], o, d, rtx.rtx.RAY_HIT_DTYPE)
    hit = exp["prim"] != NO_HIT
    assert hit.sum() >= 150 and (hit & (exp["prim"] != bunny["ground"])).sum() >= 30 and np.isfinite(exp["t"]).all()
    trace_every_way(bunny["scene"], o, d, exp, bunny["normals"], "far origins x%d" % scale)
    want = expected_occlusion(exp, o, target)
    assert want.sum() >= 50 and (want == 0).sum() >= 30
    occluded_every_way(bunny["scene"], o, target, want, "far origins x%d" % scale)
    ro, rd, rexp, _ = bunny["sets"]["random"]
    mo, md, mexp = np.empty((400, 3), F), np.empty((400, 3), F), np.empty(400, exp.dtype)
    mo[0::2], md[0::2], mexp[0::2] = o, d, exp
    mo[1::2], md[1::2], mexp[1::2] = ro[:200], rd[:200], rexp[:200]
    trace_every_way(bunny["scene"], mo, md, mexp, bunny["normals"], "far and near origins interleaved x%d" % scale)


def test_a_batch_above_the_regrouping_threshold_with_default_flags(bunny):
    """The random set repeated until it is larger than the library's threshold (16,384 rays), shuffled: with flags = 0
    the batch takes the regrouping pass, and every copy of a ray must get that ray's answer."""
    o, d, exp, _ = bunny["sets"]["random"]
    order = np.random.default_rng(3).permutation(np.tile(np.arange(len(o)), 12))
    assert len(order) == 18000 > 16384
    got, st = bunny["scene"].trace_rays(o[order], d[order], stats=True)
    check_hits(got, exp[order], bunny["normals"], "18,000 rays, default flags")
    assert st["primary_hits"] == 12 * int((exp["prim"] != NO_HIT).sum())
    assert got.tobytes() == bunny["scene"].trace_rays(o[order], d[order], keep_order=True).tobytes()
    ro, targets, rexp, _ = bunny["sets"]["random_targets"]
    want = expected_occlusion(rexp, ro, targets)[order]
    assert np.array_equal(bunny["scene"].occluded_rays(ro[order], targets[order]), want)
