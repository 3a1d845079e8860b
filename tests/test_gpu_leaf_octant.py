"""The leaf's own-box pretest under every direction octant (run with -m gpu on an MI355X).

A 32 x 32 frame of a 40-triangle cluster is lit, through the lit calls, by eight lights that each put every shadow ray
of the frame into one octant (bit a of the octant: direction component a negative, walk_octant), and by a ninth placed
directly over the cluster, so that dx and dz change sign among the rays of one chunk and the walk runs its general
copy.  A batch through rtx_occluded_rays holds rays of all eight octants in each wavefront.

  * bytes and flags are the oracle's, for the oracle scene created with that light;
  * the counted statistics of every frame and of the batch — box tests, primitive tests, both visit counts — equal the
    ones recorded with the parent commit's library in tests/golden/leaf_octant_counts.json: the pretest may be restated
    (each comparison voted on its own; near and far planes named by the octant), but it computes the same numbers, so no
    walk may visit or skip another record."""
import importlib
import json
import os

import numpy as np
import pytest

import gpu_forms as gf
import query_sets as qs

pytestmark = pytest.mark.gpu
F = np.float32
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "leaf_octant_counts.json")
W = H = 32
NB_LIGHT = 12
COUNTS = ("box_tests", "tri_tests", "wave_node_visits", "wave_tri_visits")
LIGHTS = ["octant %d" % k for k in range(8)] + ["overhead"]


def cluster(seed=44, n=40):
    rng = np.random.default_rng(seed)
    c = rng.uniform(-10.0, 10.0, size=(n, 1, 3)) + gf.OCT_CENTRE
    tris = (c + rng.uniform(-5.0, 5.0, size=(n, 3, 3))).astype(F).reshape(n, 9)
    return tris, rng.uniform(0.2, 1.0, size=(n, 3)).astype(F)


def light_tri(name):
    if name == "overhead":
        centre = gf.OCT_CENTRE + np.array([0.0, gf.OCT_LIGHT_OFFSET, 0.0])
        return (centre + np.array([[-1.0, 0.0, -1.0], [1.0, 0.2, -1.0], [0.0, -0.2, 1.5]])).astype(F).reshape(9)
    return gf.light_in_octant(int(name.split()[1]))


def camera():
    """the eye a hundred units in front of the cluster, a little off its axis: no light lies behind the eye, every light's
    shadows fall on faces the eye sees"""
    eye = gf.OCT_CENTRE + np.array([8.0, 5.0, 100.0])
    return dict(eye=tuple(float(x) for x in eye), look_at=tuple(float(x) for x in gf.OCT_CENTRE), up=(0.0, 1.0, 0.0), distance=130.0)


def octant_batch(seed=45, n=64):
    """n point pairs, ray i in octant i % 8: origins inside the cluster's box, targets beyond it on the octant's side"""
    rng = np.random.default_rng(seed)
    o = (rng.uniform(-8.0, 8.0, size=(n, 3)) + gf.OCT_CENTRE).astype(F)
    signs = np.stack([gf.octant_signs(i % 8) for i in range(n)])
    t = (gf.OCT_CENTRE + signs * (gf.OCT_LIGHT_OFFSET + rng.uniform(-3.0, 3.0, size=(n, 3)))).astype(F)
    return o, t


def measure(rtx, samples):
    """every fixture frame and the batch with statistics -> {name: {"rows" / "view" / "batch": [the four counts]}}, and the
    outputs: {name: image}, the batch's flags"""
    tris, rgb = cluster()
    counts, images = {}, {}
    pick = lambda st: [int(st[k]) for k in COUNTS]
    with rtx.Scene(W, H, tris, rgb, samples, light_tri=light_tri("octant 0"), nb_light_sample=NB_LIGHT, **camera()) as s:
        view = s.own_view()
        for name in LIGHTS:
            light = s.make_light(light_tri(name), NB_LIGHT)
            rows, st_rows = s.render_view_rows(view, light=light, stats=True)
            plain = s.render_view_rows(view, light=light)
            assert np.array_equal(rows, plain), name + ": the counted and the uncounted compilation differ"
            got, st_view = s.render_view(view, light=light, stats=True)
            assert np.array_equal(got, rows), name + ": render_view_lit and render_view_rows_lit differ"
            counts[name] = dict(rows=pick(st_rows), view=pick(st_view))
            images[name] = rows
        o, t = octant_batch()
        flags, st = s.occluded_rays(o, t, keep_order=True, stats=True)
        assert np.array_equal(flags, s.occluded_rays(o, t, keep_order=True))
        counts["batch"] = dict(batch=pick(st))
    return counts, images, flags


@pytest.fixture(scope="module")
def measured(orc, samples_seeded):
    rtx = importlib.import_module("ray-tracer-rust_amd")
    assert rtx.device_count() >= 1, "no HIP device: the product path has no CPU fallback"
    return measure(rtx, samples_seeded)


@pytest.mark.parametrize("name", LIGHTS)
def test_frames_under_each_light_are_the_oracles(orc, samples_seeded, measured, name):
    tris, rgb = cluster()
    light = np.asarray(light_tri(name), np.float64).reshape(3, 3)
    lo, hi = gf.prim_box(tris, {})
    if name == "overhead":
        assert light[:, 1].min() > hi[1] + 1.0 and (light[:, 0].min() > lo[0] + 5.0) and (light[:, 0].max() < hi[0] - 5.0) \
            and (light[:, 2].min() > lo[2] + 5.0) and (light[:, 2].max() < hi[2] - 5.0), "over the cluster, inside its x and z range"
    else:
        k = int(name.split()[1])
        for a in range(3):      # strictly beyond the box of all primitives on every axis: every shadow ray is in octant k
            assert (light[:, a].max() < lo[a] - 1.0) if (k >> a) & 1 else (light[:, a].min() > hi[a] + 1.0)
    osc = orc.Scene(W, H, tris, rgb, samples_seeded, light_tri=light_tri(name), nb_light_sample=NB_LIGHT, **camera())
    ref, ost, otri = osc.render_rows(mode=orc.MODE_BVH, want_tri=True)
    osc.close()
    hits, lit, black = gf.oracle_counts(ref, otri)
    assert hits >= 300 and lit >= 100 and black >= 10, "shadow rays must both pass and be stopped: %d %d %d" % (hits, lit, black)
    bad = int((measured[1][name] != ref).any(axis=2).sum())
    assert bad == 0, "%s: %d pixels differ from the oracle" % (name, bad)


def test_a_wavefront_with_a_ray_of_every_octant(orc, samples_seeded, measured):
    tris, rgb = cluster()
    o, t = octant_batch()
    d = t - o
    for i in range(len(o)):
        assert [bool(x < 0) for x in d[i]] == [bool((i % 8 >> a) & 1) for a in range(3)]
    osc = orc.Scene(W, H, tris, rgb, samples_seeded, light_tri=light_tri("octant 0"), nb_light_sample=NB_LIGHT, **camera())
    want = qs.pair_sets(orc, osc, o, t)["occlusion"][3]
    osc.close()
    assert want.sum() >= 8 and (want == 0).sum() >= 8
    assert np.array_equal(measured[2], want)


def test_the_walks_visit_the_records_the_parent_commit_visited(measured):
    with open(GOLDEN) as f:
        golden = json.load(f)
    assert sorted(golden["counts"]) == sorted(measured[0])
    for name, per_call in measured[0].items():
        for call, got in per_call.items():
            assert got == golden["counts"][name][call], "%s, %s: %s = %s, recorded %s" % (name, call, COUNTS, got, golden["counts"][name][call])
            assert got[1] > 0 and got[3] > 0
