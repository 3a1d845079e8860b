"""Each compiled form of the kernels against the oracle, every byte (run with -m gpu on an MI355X).

librtx.so holds probe_kernel / shade_tiles_kernel for each of COUNT x SPHERES x WHOLE and reference_tiles_kernel for
COUNT x SPHERES (tests/gpu_forms.py names the switches), and advance_to_leaf holds nine hand-written box loops.  The
other GPU modules run the cut forms (WHOLE = false) on their edge scenes, both counting states through render_both;
this module runs
  * the whole-stream forms (WHOLE = true) of librtx.so itself: without and with spheres, two primary rays per pixel,
    tiles queued for reference_tiles_kernel — each test asserts that its stream has more than 65,536 records;
  * each box loop by name: 16 scenes whose primary directions and whose surface-to-light directions are shown, from the
    inputs alone, to lie in one stated octant, and two scenes where no octant is common (the general loop).
Every scene renders with and without statistics (render_both) and the uncounted image is the one compared."""
import importlib

import numpy as np
import pytest

import gpu_forms as gf

pytestmark = pytest.mark.gpu
F = np.float32


@pytest.fixture(scope="module")
def rtx():
    mod = importlib.import_module("ray-tracer-rust_amd")
    assert mod.device_count() >= 1, "no HIP device: the product path has no CPU fallback"
    return mod


def same_bytes(img, ref, what):
    assert img.shape == ref.shape, what
    bad = (img != ref).any(axis=2)
    ys, xs = np.nonzero(bad)
    tiles = sorted({(int(x) // 8, int(y) // 8) for x, y in zip(xs, ys)})
    print("%s: %d of %d pixels differ" % (what, int(bad.sum()), bad.size))
    assert not bad.any(), "%s: %d pixels differ from the oracle; 8 x 8 tiles (x, y): %s" % (what, int(bad.sum()), tiles[:12])


# ------------------------------------------------------------------------------------------- whole-stream forms
@pytest.mark.parametrize("n_spheres,nb_ray", [(0, 1), (300, 1), (0, 2), (300, 2)],
                         ids=["triangles", "spheres", "triangles-nb_ray2", "spheres-nb_ray2"])
def test_whole_stream_forms_match_the_oracle(rtx, orc, samples_seeded, n_spheres, nb_ray):
    """probe_kernel / shade_tiles_kernel<COUNT, SPHERES, WHOLE = true> for both COUNT (render_both) and both SPHERES:
    35,000 synthetic triangles + the ground, one primitive per leaf -> 70,001 records, above the 65,536 up to which
    tiles get cuts of their own.  With nb_ray = 2 the running sums cross HBM between the passes.  No reference tree at
    this size: the checker is the oracle's leaf-gated brute force (equal to its faithful BVH where no ray has a -0.0
    direction component and no exact tie occurs; ties and non-finite distances asserted absent)."""
    W, H, L = 40, 32, 8
    tris, rgb, extra = gf.whole_stream_scene(rtx, n_spheres=n_spheres)
    osc = orc.Scene(W, H, tris, rgb, samples_seeded, nb_ray=nb_ray, nb_light_sample=L, build_bvh=False, **extra)
    ref, ost, otri = osc.render_rows(mode=orc.MODE_LEAFBOX, want_tri=True)
    assert ost["exact_ties"] == 0 and ost["nonfinite_t"] == 0
    hits, lit, black = gf.oracle_counts(ref, otri)
    assert hits > 500 and lit > 200
    if n_spheres:
        arm = extra["kinds"][otri[otri != gf.NO_HIT]]
        assert (arm == 1).sum() >= 50 and (arm == 0).sum() >= 50, "both arms must be seen"
    with rtx.Scene(W, H, tris, rgb, samples_seeded, nb_ray=nb_ray, nb_light_sample=L, leaf_max=1,
                   reference_tree=rtx.REFTREE_NEVER, tie_rank=None, **extra) as s:
        info = s.info()
        assert info["n_nodes"] > gf.CUT_MAX_NODES and info["n_ref_nodes"] == 0, info
        img, st = gf.render_both(s)
    assert st["primary_rays"] == nb_ray * W * H and st["primary_hits"] == ost["primary_hits"]
    assert st["redo_tiles"] == 0
    same_bytes(img, ref, "whole stream, %d spheres, nb_ray %d" % (n_spheres, nb_ray))


@pytest.mark.parametrize("n_spheres", [0, 300], ids=["triangles", "spheres"])
def test_whole_stream_with_tiles_queued_for_the_reference_walk(rtx, orc, n_spheres):
    """WHOLE = true with reference_tiles_kernel<COUNT, SPHERES> at work: the soup moved in front of an axis-aligned
    camera at the origin, an all-zero sample table (exact zeros in the directions of the centre row and column: those
    tiles are queued), the reference tree built.  32,800 triangles + the ground at one per leaf: 65,601 records (65,537
    is the least that runs the whole-stream form); the oracle builds its O(n^2) tree for them in about 1.3 s of
    one CPU core, the library in as much again.  Checker: the oracle's faithful BVH."""
    W = H = 32
    tris, rgb, extra = gf.whole_stream_scene(rtx, n=gf.WHOLE_N_QUEUED, n_spheres=n_spheres)
    n_prims = len(tris) + n_spheres
    tris, extra = gf.into_axis_view(tris, extra)
    assert len(tris) + n_spheres == n_prims == gf.WHOLE_N_QUEUED + 1 + n_spheres
    T = np.zeros((4096, 2), F)
    kw = dict(gf.AXIS_CAMERA, nb_light_sample=8)
    ref, ost, otri = orc.Scene(W, H, tris, rgb, T, **extra, **kw).render_rows(mode=orc.MODE_BVH, want_tri=True)
    assert ost["nonfinite_t"] == 0 and ost["primary_hits"] > 300
    if n_spheres:
        arm = extra["kinds"][otri[otri != gf.NO_HIT]]
        assert (arm == 1).sum() >= 20 and (arm == 0).sum() >= 50
    with rtx.Scene(W, H, tris, rgb, T, leaf_max=1, reference_tree=rtx.REFTREE_ALWAYS, **extra, **kw) as s:
        info = s.info()
        assert info["n_nodes"] > gf.CUT_MAX_NODES and info["n_ref_nodes"] == 2 * n_prims - 1, info
        img, st = gf.render_both(s)
    assert st["redo_tiles"] > 0
    assert st["primary_hits"] == ost["primary_hits"]
    same_bytes(img, ref, "whole stream with queued tiles, %d spheres" % n_spheres)


# ------------------------------------------------------------------------------------------- the nine box loops
def _render_and_compare(rtx, orc, samples, scene):
    """Oracle (faithful BVH) and product, both counting states; the scene only counts if the oracle alone shows enough
    hits, lit pixels and shadowed pixels.  -> the oracle's want_tri plane"""
    name, W, H, tris, rgb, extra, kw = scene
    ref, ost, otri = orc.Scene(W, H, tris, rgb, samples, **extra, **kw).render_rows(mode=orc.MODE_BVH, want_tri=True)
    hits, lit, black = gf.oracle_counts(ref, otri)
    print("%s: oracle hits %d, lit %d, hit and black %d" % (name, hits, lit, black))
    assert ost["nonfinite_t"] == 0
    assert hits >= 300 and lit >= 100 and black >= 20, "shadow rays must both pass and be stopped"
    if extra:
        arm = extra["kinds"][otri[otri != gf.NO_HIT]]
        assert (arm == 1).sum() >= 50 and (arm == 0).sum() >= 50
    with rtx.Scene(W, H, tris, rgb, samples, **extra, **kw) as s:
        assert s.info()["n_global"] == 0                # no floor: nothing is tested outside the tree
        img, st = gf.render_both(s)
    assert st["primary_hits"] == ost["primary_hits"] == hits
    same_bytes(img, ref, name)
    return otri


@pytest.mark.parametrize("eye_oct,light_oct,with_spheres", gf.OCTANT_CASES,
                         ids=["eye%d-light%d%s" % (e, l, "-spheres" if s else "") for e, l, s in gf.OCTANT_CASES])
def test_box_loop_of_each_octant(rtx, orc, samples_seeded, eye_oct, light_oct, with_spheres):
    """advance_to_leaf's loop `eye_oct` under the primary rays (closest hit) and loop `light_oct` under the shadow
    rays (any hit), in the sense of walk_octant: bit a of the octant set = direction component a negative.  Shown from
    the inputs: every primary direction of the frame has the eye octant's signs, and the light triangle's box lies
    strictly beyond the box of all primitives on every axis, on the light octant's side."""
    scene = gf.octant_scene(eye_oct, light_oct, with_spheres)
    name, W, H, tris, rgb, extra, kw = scene
    lo, hi = gf.prim_box(tris, extra)
    light = np.asarray(kw["light_tri"], np.float64).reshape(3, 3)
    for a in range(3):
        if (light_oct >> a) & 1:
            assert light[:, a].max() < lo[a] - 1.0, "axis %d: the light must lie below the soup" % a
        else:
            assert light[:, a].min() > hi[a] + 1.0, "axis %d: the light must lie above the soup" % a
    d = gf.primary_directions(rtx, W, H, samples_seeded, kw)
    for a in range(3):
        assert ((d[..., a] < 0.0) if (eye_oct >> a) & 1 else (d[..., a] > 0.0)).all(), "axis %d of the primary rays" % a
    _render_and_compare(rtx, orc, samples_seeded, scene)


@pytest.mark.parametrize("which", gf.GENERAL_CASES, ids=[w.replace(" ", "-") for w in gf.GENERAL_CASES])
def test_general_box_loop_where_no_octant_is_common(rtx, orc, samples_seeded, which):
    """Loop 8 as the only choice.  The light triangle lies inside the soup: per pixel, the box of the primitive the
    oracle hits lies wholly on one side of the light's box or the other, which fixes the sign of the shadow rays from
    that pixel; both signs occur on every axis, and inside single 8 x 8 tiles.  In the second scene the eye is inside
    as well and the primary directions of the centre tile have both signs on x and on y."""
    scene = gf.general_loop_scene(which)
    name, W, H, tris, rgb, extra, kw = scene
    lo, hi = gf.prim_box(tris, extra)
    light = np.asarray(kw["light_tri"], np.float64).reshape(3, 3)
    assert (light.min(axis=0) > lo + 5.0).all() and (light.max(axis=0) < hi - 5.0).all(), "the light is inside the soup"
    d = gf.primary_directions(rtx, W, H, samples_seeded, kw)
    if which == "eye and light inside":
        assert (np.asarray(kw["eye"]) > lo + 5.0).all() and (np.asarray(kw["eye"]) < hi - 5.0).all()
        ty, tx = (H // 2) // 8 * 8, (W // 2) // 8 * 8
        centre = d[ty:ty + 8, tx:tx + 8]
        for a in (0, 1):
            assert (centre[..., a] < 0.0).any() and (centre[..., a] > 0.0).any(), "axis %d of the centre tile" % a
    otri = _render_and_compare(rtx, orc, samples_seeded, scene)
    plo, phi = gf.hit_prim_boxes(tris, extra, otri)
    with np.errstate(invalid="ignore"):
        towards_plus = phi < light.min(axis=0)          # the surface lies below the light: direction component > 0
        towards_minus = plo > light.max(axis=0)
    mixed_tiles = 0
    for a in range(3):
        assert towards_plus[..., a].sum() >= 20 and towards_minus[..., a].sum() >= 20, "axis %d of the shadow rays" % a
    for ty in range(0, H, 8):
        for tx in range(0, W, 8):
            p, m = towards_plus[ty:ty + 8, tx:tx + 8], towards_minus[ty:ty + 8, tx:tx + 8]
            mixed_tiles += bool((p.any(axis=(0, 1)) & m.any(axis=(0, 1))).any())
    assert mixed_tiles >= 10, "tiles whose shadow rays differ in sign on some axis"
