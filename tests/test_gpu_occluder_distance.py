"""The shadow walk's distance test on the GPU (run with -m gpu on an MI355X): the fixtures of tests/occluder_sets.py —
candidates the certificate settles either way, candidates within ulps of the light's distance, and both kinds in one
wavefront — through rtx_occluded_rays (flags, ray by ray against the oracle), rtx_shade_rays and the three render entry
points, with one and two primary rays per pixel, with and without a sphere in the scene, and in the whole-stream form.
Zero differing bytes and flags."""
import importlib

import numpy as np
import pytest

import gpu_forms as gf
import occluder_sets as oc
import shade_sets as ss

pytestmark = pytest.mark.gpu
F = np.float32
CASES = [(name, nb_ray, sphere) for name in oc.FIXTURES for nb_ray in (1, 2) for sphere in (False, True)]


@pytest.fixture(scope="module")
def rtx():
    mod = importlib.import_module("ray-tracer-rust_amd")
    assert mod.device_count() >= 1, "no HIP device: the product path has no CPU fallback"
    return mod


def differing(a, b):
    assert a.shape == b.shape
    return int((a != b).any(axis=-1).sum())


@pytest.mark.parametrize("name,nb_ray,sphere", CASES, ids=["%s-nb_ray%d%s" % (n, r, "-sphere" if s else "") for n, r, s in CASES])
def test_frames_and_shaded_rays_are_the_oracles_bytes(rtx, orc, samples_seeded, name, nb_ray, sphere):
    f = oc.fixture(name, nb_ray=nb_ray, sphere=sphere)
    W, H = f["W"], f["H"]
    osc = orc.Scene(W, H, f["tris"], f["rgb"], samples_seeded, **f["extra"], **f["kw"])
    ref, ost = osc.render_rows(mode=orc.MODE_BVH)
    osc.close()
    lit = ref.max(axis=2) > 0
    if name == "beyond":
        assert lit.all()
    else:
        assert lit.any() and (~lit).any()
    o, raw, _, _, _ = ss.camera_raw_rays(orc, W, H, f["kw"]["eye"], f["kw"]["look_at"], f["kw"]["up"], f["kw"]["distance"],
                                         samples_seeded, nb_ray=nb_ray)
    with rtx.Scene(W, H, f["tris"], f["rgb"], samples_seeded, **f["extra"], **f["kw"]) as s:
        img, st = gf.render_both(s)                                     # the render pipeline, counted and uncounted
        assert st["primary_hits"] == ost["primary_hits"]
        assert differing(img, ref) == 0, "render_rows"
        view = s.own_view()
        got, shade = s.render_view(view, want_shade=True)
        assert differing(got, ref) == 0, "render_view"
        assert differing(s.render_view_rows(view), ref) == 0, "render_view_rows"
        assert s.render_view_rows_shade(view).tobytes() == shade.tobytes(), "render_view_rows_shade"
        for mode in (dict(keep_order=True), dict(), dict(force_regroup=True)):
            rec = s.shade_rays(o, raw, **mode)
            assert differing(rec["rgb8"].reshape(H, W, 3), ref) == 0, ("shade_rays", mode)
            assert rec.tobytes() == shade.tobytes(), ("shade_rays and render_view", mode)


@pytest.mark.parametrize("name", oc.FIXTURES)
def test_occlusion_flags_ray_by_ray(rtx, orc, samples_seeded, name):
    s = oc.shadow_rays(orc, samples_seeded, name)
    f = s["fixture"]
    want = s["occluded"]
    with rtx.Scene(f["W"], f["H"], f["tris"], f["rgb"], samples_seeded, **f["kw"]) as scene:
        for mode in (dict(keep_order=True), dict(), dict(force_regroup=True)):
            for stats in (False, True):
                got = scene.occluded_rays(s["origins"], s["targets"], stats=stats, **mode)
                if stats:
                    got, st = got
                    assert st["primary_hits"] == int(want.sum())
                assert np.array_equal(got, want), "%s %s: %d flags differ" % (name, mode, int((got != want).sum()))
        # a light point's 64 rays as one wavefront, in the caller's order: settled and unsettled lanes side by side
        if name == "tile":
            for k in range(oc.NB_LIGHT):
                got = scene.occluded_rays(s["origins"][k::oc.NB_LIGHT], s["targets"][k::oc.NB_LIGHT], keep_order=True)
                assert np.array_equal(got, want[k::oc.NB_LIGHT]), "light point %d" % k


FILLER = 33000


@pytest.mark.parametrize("name,sphere", [("tile", False), ("coplanar", True)], ids=["tile", "coplanar-sphere"])
def test_whole_stream_form(rtx, orc, samples_seeded, name, sphere):
    """the same pixels with 33,000 small triangles far below the view added, one primitive per leaf: more than 65,536
    stream records, so every chunk walks the whole stream (probe_kernel / shade_tiles_kernel<.., WHOLE = true>).  The
    checker is the oracle's leaf-gated brute force (no tie and no non-finite distance, asserted)."""
    f = oc.fixture(name, sphere=sphere)
    rng = np.random.default_rng(17)
    c = rng.uniform(-50.0, 50.0, size=(FILLER, 1, 3)) + np.array([0.0, -400.0, -20.0])
    filler = (c + rng.uniform(-0.5, 0.5, size=(FILLER, 3, 3))).astype(F).reshape(FILLER, 9)
    tris = np.ascontiguousarray(np.concatenate([filler, f["tris"]]))
    rgb = np.ascontiguousarray(np.concatenate([np.ones((FILLER, 3), F), f["rgb"]]))
    W, H = f["W"], f["H"]
    osc = orc.Scene(W, H, tris, rgb, samples_seeded, build_bvh=False, **f["extra"], **f["kw"])
    ref, ost = osc.render_rows(mode=orc.MODE_LEAFBOX)
    osc.close()
    assert ost["exact_ties"] == 0 and ost["nonfinite_t"] == 0
    small = oc.shadow_rays(orc, samples_seeded, name)["image"]
    assert differing(ref, small) == 0, "the added triangles change no pixel"
    with rtx.Scene(W, H, tris, rgb, samples_seeded, leaf_max=1, reference_tree=rtx.REFTREE_NEVER, tie_rank=None,
                   **f["extra"], **f["kw"]) as s:
        assert s.info()["n_nodes"] > gf.CUT_MAX_NODES
        img, st = gf.render_both(s)
    assert st["primary_hits"] == ost["primary_hits"]
    assert differing(img, ref) == 0
