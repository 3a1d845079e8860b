"""GPU parity of the ray-query entry points on the paths only a caller's rays reach: scenes holding spheres (occlusion
queries, origins inside a sphere, far origins, hard rays), occlusion targets on and one ulp beside the hit point, hard
rays on each axis and in several groups, a hard ray beside a far origin, directions scaled by powers of two across
length_and_direction's whole-wavefront gates, and batch sizes around a key_kernel workgroup.  The ray sets and the
oracle's answers are tests/query_sets.py's (their conditions: tests/test_query_sets.py); every set is traced in the
caller's order, in the default mode and with the regrouping pass forced, with and without statistics, and compared bit
for bit: primitive, t, p_hit, normal, occlusion byte.  No tolerance anywhere."""
import importlib
import os

import numpy as np
import pytest

import query_sets as qs
from test_gpu_trace_rays import occluded_every_way, trace_every_way

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def rtx():
    mod = importlib.import_module("ray-tracer-rust_amd")
    assert mod.device_count() >= 1, "no HIP device: the product path has no CPU fallback"
    assert mod.rtx.RAY_HIT_DTYPE == qs.HIT_DTYPE
    return mod


@pytest.fixture(scope="module")
def sets(orc, samples_seeded):
    return lambda name: getattr(qs, name)(orc, samples_seeded)


@pytest.fixture(scope="module")
def bunny(rtx, samples_seeded):
    """big_bunny + ground, reference tree built"""
    scene = rtx.default_scene([os.path.join(ROOT, "models", "big_bunny.obj")], qs.W, qs.H, samples_seeded)
    assert scene.info()["n_tris"] == 4969 and scene.info()["n_ref_nodes"] != 0
    yield dict(scene=scene, normals=scene.normals())
    scene.close()


@pytest.fixture(scope="module")
def soup(rtx, sets):
    """scene A: 220 triangles and 60 spheres, reference tree built"""
    a = sets("scene_a")
    scene = rtx.Scene(*a["args"], **a["kw"])
    assert scene.info()["n_tris"] == 280 and scene.info()["n_ref_nodes"] != 0
    yield dict(scene=scene, stored=scene.normals(), kinds=a["kinds"])
    scene.close()


def trace_soup(soup, ray_set, what):
    o, d, exp, _ = ray_set
    got = trace_every_way(soup["scene"], o, d, exp, None, what)
    qs.check_normals(got, exp, soup["stored"], soup["kinds"], what)
    return got


def redo_tiles(call, first, second, **mode):
    _, st = call(first, second, stats=True, **mode)
    return st["redo_tiles"]


def test_a_mixed_soup_with_spheres(rtx, sets, soup):
    """closest hit and occlusion on a scene holding spheres (occluded_kernel<., SPHERES = true>), 60 origins inside a
    sphere; the brute-force build of the scene gives the same bytes"""
    a, s = sets("scene_a"), sets("set_a")
    got = trace_soup(soup, s["trace"], "A")
    o, t, _, want = s["occlusion"]
    occluded_every_way(soup["scene"], o, t, want, "A")
    kw = dict(a["kw"], accel=1)
    with rtx.Scene(*a["args"], **kw) as brute:
        for mode in (dict(keep_order=True), dict(force_regroup=True)):
            assert brute.trace_rays(o, s["trace"][1], **mode).tobytes() == got.tobytes(), mode
            assert np.array_equal(brute.occluded_rays(o, t, **mode), want), mode


@pytest.mark.parametrize("which", ["far", "mixed"])
def test_b_far_origins_on_the_sphere_scene(sets, soup, which):
    """the exact-slab walk (closest_hit / any_hit<., false, true>) over sphere leaves: far origins alone, and
    interleaved one for one with near ones"""
    b = sets("set_b")[which]
    trace_soup(soup, b["trace"], "B " + which)
    o, t, _, want = b["occlusion"]
    occluded_every_way(soup["scene"], o, t, want, "B " + which)


def test_c_hard_rays_on_three_axes_in_three_groups(sets, bunny):
    """-0.0 in x, y and z at slots 0, 127 and 149 of 150: three groups take the reference walk in the caller's order, one
    after the regrouping pass (key bit 31 sorts the three into slots 147-149, all in group 2)"""
    c, scene = sets("set_c")["bunny"], bunny["scene"]
    o, d, exp, _ = c["trace"]
    trace_every_way(scene, o, d, exp, bunny["normals"], "C bunny")
    assert redo_tiles(scene.trace_rays, o, d, keep_order=True) == 3
    assert redo_tiles(scene.trace_rays, o, d, force_regroup=True) == 1
    o, t, _, want = c["occlusion"]
    occluded_every_way(scene, o, t, want, "C bunny")
    assert redo_tiles(scene.occluded_rays, o, t, keep_order=True) == 3
    assert redo_tiles(scene.occluded_rays, o, t, force_regroup=True) == 1


def test_c_hard_ray_on_the_sphere_scene(sets, soup):
    """closest_hit_reference<., SPHERES = true> and the occlusion branch behind it: one group of 64, a -0.0 ray in it"""
    c, scene = sets("set_c")["scene_a"], soup["scene"]
    trace_soup(soup, c["trace"], "C scene A")
    o, t, _, want = c["occlusion"]
    occluded_every_way(scene, o, t, want, "C scene A")
    for mode in (dict(keep_order=True), dict(force_regroup=True)):
        assert redo_tiles(scene.trace_rays, c["trace"][0], c["trace"][1], **mode) == 1, mode
        assert redo_tiles(scene.occluded_rays, o, t, **mode) == 1, mode


def test_c_hard_ray_and_far_origin_in_one_group(sets, bunny):
    """both votes of the wavefront fire: the far origin asks for the exact-slab walk, the hard ray sends the group
    through the reference walk; all 64 get the oracle's answers"""
    c, scene = sets("set_c")["both"], bunny["scene"]
    o, d, exp, _ = c["trace"]
    trace_every_way(scene, o, d, exp, bunny["normals"], "C both")
    assert redo_tiles(scene.trace_rays, o, d, keep_order=True) == 1
    o, t, _, want = c["occlusion"]
    occluded_every_way(scene, o, t, want, "C both")
    assert redo_tiles(scene.occluded_rays, o, t, keep_order=True) == 1


@pytest.mark.parametrize("where", ["at", "toward", "away"])
def test_d_occlusion_with_the_target_at_the_hit_point(sets, bunny, soup, where):
    """candidate_occludes where it is tight: distance(origin, p_hit) and the distance to the target are equal or one ulp
    apart, and any_hit may meet a farther surface before the closest one"""
    d = sets("set_d")
    o, t, _, want = d["bunny"]["targets"][where]
    occluded_every_way(bunny["scene"], o, t, want, "D bunny " + where)
    o, t, _, want = d["scene_a"]["targets"][where]
    occluded_every_way(soup["scene"], o, t, want, "D scene A " + where)


@pytest.mark.parametrize("batch", ["2^-60", "2^-36", "2^49", "2^52", "one_lane"])
def test_e_direction_scales(sets, bunny, batch):
    """length_and_direction's two ways give the same bits: the scaled rays get the unscaled rays' records, whether the
    whole batch, some lanes or one lane of each wavefront lies beyond a gate"""
    e = sets("set_e")
    o, d, exp, _ = e["trace"][batch]
    trace_every_way(bunny["scene"], o, d, exp, bunny["normals"], "E " + batch)
    if batch in e["occlusion"]:
        o, t, _, want = e["occlusion"][batch]
        occluded_every_way(bunny["scene"], o, t, want, "E " + batch)


@pytest.mark.parametrize("n", [255, 256, 257])
def test_f_batch_sizes_around_a_key_kernel_workgroup(sets, bunny, n):
    b = sets("bunny")["sets"]
    o, d, exp, _ = b["random"]
    trace_every_way(bunny["scene"], o[:n], d[:n], exp[:n], bunny["normals"], "random[:%d]" % n)
    o, t, texp, _ = b["random_targets"]
    want = qs.expected_occlusion(texp, o, t)
    occluded_every_way(bunny["scene"], o[:n], t[:n], want[:n], "random pairs[:%d]" % n)
