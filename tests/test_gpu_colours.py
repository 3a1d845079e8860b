"""GPU parity of colours (run with -m gpu on an MI355X): pixels whose linear value lies AT each of the 255 gamma steps and
one float below it, and primitive colours of every class a caller may hand in — zeros of both signs, negatives, huge and
tiny values, infinities, NaN (tests/colour_sets.py, whose conditions tests/test_colour_sets.py asserts without a GPU).
The expected values are those of an ORACLE SCENE CREATED WITH THE COLOURS; every comparison is for zero differing bytes or
words, and where the oracle's linear value is NaN the device's must be a NaN too (degenerate_sets.same_floats).

What these tests cannot see: the bits of div_denom's fall-back quotient for a numerator outside [2^-60, 2^60] — such sums
quantise to 0 or 255 and their linear words are compared only through the view and shade kernels, which divide outright.
The tests pin that path's bytes and the bytes and linear words of the in-range pixels that share its wavefronts."""
import importlib
import time

import numpy as np
import pytest

import colour_sets as cs
import degenerate_sets as dg
import gpu_forms as gf
import light_sets as ls
import shade_sets as ss
import view_sets as vs
from query_sets import F, NO_HIT, bits

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def rtx():
    mod = importlib.import_module("ray-tracer-rust_amd")
    assert mod.device_count() >= 1, "no HIP device: the product path has no CPU fallback"
    return mod


class Tally:
    """counts the comparisons of a test and the bytes or words that differ in them; check() asserts that none does"""

    def __init__(self, what):
        self.what, self.n, self.bad, self.first, self.t0 = what, 0, 0, None, time.perf_counter()

    def same(self, got, want, what):
        got, want = np.asarray(got), np.asarray(want)
        assert got.shape == want.shape, (what, got.shape, want.shape)
        differ = int((got != want).sum())
        self.n += 1
        self.bad += differ
        if differ:
            print("    %s: %d differ" % (what, differ))
        if differ and self.first is None:
            self.first = "%s at %s: %s, expected %s" % (what, np.argwhere(got != want)[:4].tolist(), got[got != want][:4], want[got != want][:4])

    def same_floats(self, got, want, what):
        """equal bits, or a NaN on both sides"""
        got, want = np.ascontiguousarray(got, F), np.ascontiguousarray(want, F)
        try:
            dg.same_floats(got, want, True, what)
            self.n += 1
        except AssertionError as e:
            self.n += 1
            self.bad += int(((bits(got) != bits(want)) & ~(np.isnan(got) & np.isnan(want))).sum())
            self.first = self.first or str(e)
            print("    %s: %s" % (what, e))

    def check(self):
        print("%s: %d comparisons, %d differing bytes or words, %.2f s" % (self.what, self.n, self.bad, time.perf_counter() - self.t0))
        assert self.bad == 0, "%s: %d bytes or words differ; first: %s" % (self.what, self.bad, self.first)


def lib_view(rtx, frame, camera):
    return rtx.Scene.view(frame[0], frame[1], **camera)


def ground_camera(orc, distance):
    return dict(eye=orc.EYE, look_at=orc.LOOK_AT, up=orc.UP, distance=distance)


def primary_rays(orc, frame, camera, samples, nb_ray):
    o, d, _, _, _ = ss.camera_raw_rays(orc, frame[0], frame[1], camera["eye"], camera["look_at"], camera["up"], camera["distance"],
                                       samples[:4096], nb_ray)
    return o, d


def posed_frame(tally, scene, view, frame, lin, what, nan=False):
    """the posed pipeline call and the posed view call with its shade records against one oracle frame"""
    tally.same(scene.render_view_rows(view, posed=True), frame, what + ": posed rows")
    rgb, shade = scene.render_view(view, want_shade=True, posed=True)
    tally.same(rgb, frame, what + ": posed view")
    tally.same(shade["rgb8"], frame, what + ": posed view's records")
    if nan:
        tally.same_floats(shade["linear"], lin, what + ": posed view's linear")
    else:
        tally.same(bits(shade["linear"]), bits(lin), what + ": posed view's linear")


def shaded(tally, scene, o, d, frame, lin, n_hit, what, **kw):
    """rtx_shade_rays on a frame's primary rays, in the caller's order and regrouped"""
    h, w = frame.shape[:2]
    for order in (dict(keep_order=True), dict(force_regroup=True)):
        s = scene.shade_rays(o, d, **order, **kw).reshape(h, w)
        tally.same(s["rgb8"], frame, "%s: shaded rays %s" % (what, order))
        tally.same_floats(s["linear"], lin, "%s: shaded rays' linear %s" % (what, order))
        if n_hit is not None:
            tally.same(s["hits"], n_hit, "%s: shaded rays' hit counts %s" % (what, order))


# ---------------------------------------------------------------------------------------------- 1: the gamma ladder
@pytest.mark.parametrize("kind", ["grey", "coloured"])
@pytest.mark.parametrize("count", cs.LADDER_COUNTS)
def test_the_ladder_through_the_posed_pipeline_and_the_posed_view(rtx, orc, samples_seeded, count, kind):
    """One uploaded scene per sample count (the ground at 0.5); every ladder colour is given by rtx_scene_pose_prims (rgb
    alone, the vertices as uploaded) and read through rtx_render_view_rows_posed — the shading pass, its LDS copy of the
    thresholds, the grey store's one search or the three of store_pixel — and through rtx_render_view_posed with shade
    records (the view kernel's search).  All 255 steps, c_hi and c_lo, for both counts: nothing is thinned."""
    frames = cs.ladder_frames(orc, samples_seeded, count, kind)
    assert len(frames) == (510 if kind == "grey" else 170)
    tally = Tally("%s ladder, %d samples, %d colours" % (kind, count, len(frames)))
    with cs.ground_scene(rtx, samples_seeded, (0.5, 0.5, 0.5), count, reference_tree=rtx.REFTREE_NEVER, tie_rank=None) as scene:
        views = {d: lib_view(rtx, (cs.LADDER_W, cs.LADDER_H), ground_camera(orc, d)) for d in cs.LADDER_DISTANCES}
        for what, rgb, frame, lin, e in frames:
            scene.pose_prims(rgb=rgb.reshape(1, 3))
            posed_frame(tally, scene, views[e["distance"]], frame, lin, what)
    tally.check()


@pytest.mark.parametrize("count", cs.LADDER_COUNTS)
def test_every_16th_step_on_fresh_scenes_and_as_shaded_rays(rtx, orc, samples_seeded, count):
    """rtx_render_rows with and without statistics on a scene CREATED with the colour (the scene's own thresholds, planes
    and aimed stream), and rtx_shade_rays on the frame's primary rays (the shade kernel's search)"""
    frames = cs.ladder_frames(orc, samples_seeded, count, "grey", 16) + cs.ladder_frames(orc, samples_seeded, count, "coloured")[::16]
    tally = Tally("fresh scenes, %d samples, %d colours" % (count, len(frames)))
    for what, rgb, frame, lin, e in frames:
        with cs.ground_scene(rtx, samples_seeded, rgb, count, e["distance"], reference_tree=rtx.REFTREE_NEVER, tie_rank=None) as scene:
            img, st = gf.render_both(scene)
            tally.same(img, frame, what + ": rows")
            o, d = primary_rays(orc, (cs.LADDER_W, cs.LADDER_H), ground_camera(orc, e["distance"]), samples_seeded, 1)
            shaded(tally, scene, o, d, frame, lin, None, what)
    tally.check()


def test_the_scheduling_pass_stores_ladder_values_from_the_running_sums(rtx, orc, samples_seeded):
    """Two rays per pixel; the frame's one tile has a hit on ray 0 and none on ray 1 (asserted with the oracle here and in
    test_colour_sets), so the last ray's scheduling pass stores the pixels from W.acc: 16 steps, c_hi and c_lo."""
    h = cs.horizon(orc, samples_seeded)
    assert (h["hits"][:, :, 0] != NO_HIT).any() and (h["hits"][:, :, 1] == NO_HIT).all()
    tally = Tally("horizon, %d colours" % len(h["frames"]))
    more = dict(reference_tree=rtx.REFTREE_NEVER, tie_rank=None)
    view = lib_view(rtx, (cs.LADDER_W, cs.LADDER_H), ground_camera(orc, h["distance"]))
    with cs.horizon_scene(rtx, samples_seeded, (0.5, 0.5, 0.5), h["distance"], **more) as scene:
        for what, rgb, frame, lin in h["frames"]:
            scene.pose_prims(rgb=rgb.reshape(1, 3))
            posed_frame(tally, scene, view, frame, lin, what)
            with cs.horizon_scene(rtx, samples_seeded, rgb, h["distance"], **more) as fresh:
                tally.same(gf.render_both(fresh)[0], frame, what + ": rows of a fresh scene")
    tally.check()


# ---------------------------------------------------------------------------------------------- 2: colour classes
def on_device(torch, given):
    keep = {k: torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0") for k, a in given.items() if a is not None and len(a)}
    torch.cuda.synchronize()
    names = dict(v0v1v2="d_v0v1v2_ptr", spheres="d_spheres_ptr", rgb="d_rgb_ptr", sphere_rgb="d_sphere_rgb_ptr")
    kw = {names[k]: t.data_ptr() for k, t in keep.items()}
    kw.setdefault("d_v0v1v2_ptr", None)
    return kw, keep


def hit_counts(r):
    return np.minimum((r["hits"] != NO_HIT).sum(axis=2), 255).astype(np.uint8)


@pytest.mark.parametrize("nb_ray,nb_light", cs.CLASS_CONFIGS)
@pytest.mark.parametrize("ground", list(cs.GROUND_VARIANTS))
def test_a_scene_created_with_the_class_colours(rtx, orc, samples_seeded, ground, nb_ray, nb_light):
    """every entry point that renders an uploaded scene: rows counted and uncounted, the view with its records, the view
    through the pipeline, shaded rays in the caller's order and regrouped"""
    r = cs.class_render(orc, samples_seeded, ground, nb_ray, nb_light)
    tally = Tally("classes, ground %s, nb_ray %d, %d samples" % (ground, nb_ray, nb_light))
    camera = vs.camera(cs.CLASS_VIEW)
    view = lib_view(rtx, cs.CLASS_FRAME, camera)
    with cs.class_scene(rtx, samples_seeded, r["prims"], nb_ray, nb_light, reference_tree=rtx.REFTREE_NEVER, tie_rank=None) as scene:
        img, st = gf.render_both(scene)
        tally.same(img, r["frame"], "rows")
        assert st["primary_hits"] == r["stats"]["primary_hits"] and st["shadow_rays"] == r["stats"]["shadow_rays"], st
        # tile (2, 1) — descriptor 8 * 1 + 2 of the launch's one block — is full, numbered sample-major and has an empty cut:
        # the open-ground loop's kind, which a 2^61 or +inf ground leaves at its first chunk
        hits_of, flags = scene.tile_descs()[8 * 1 + 2, 1:3]
        assert hits_of == 64 and flags & 1 and (flags >> 8) & 0xFF == 0, (hits_of, hex(flags))
        rgb, shade, hits = scene.render_view(view, want_shade=True, want_hits=True)
        tally.same(rgb, r["frame"], "view")
        tally.same(shade["rgb8"], r["frame"], "view's records")
        tally.same_floats(shade["linear"], r["lin"], "view's linear")
        tally.same(shade["hits"], hit_counts(r), "view's hit counts")
        tally.same(hits["prim"], r["hits"], "view's hit primitives")
        tally.same(scene.render_view_rows(view), r["frame"], "view rows")
        o, d = primary_rays(orc, cs.CLASS_FRAME, camera, samples_seeded, nb_ray)
        shaded(tally, scene, o, d, r["frame"], r["lin"], hit_counts(r), "classes")
    tally.check()


@pytest.mark.parametrize("nb_ray,nb_light", [(2, 4), (1, 100)])
@pytest.mark.parametrize("ground", list(cs.GROUND_VARIANTS))
def test_class_colours_given_by_a_pose(rtx, orc, samples_seeded, ground, nb_ray, nb_light):
    """The scene is uploaded with ordinary colours; rtx_scene_pose_prims gives it the class colours (refitted and
    RTX_POSE_REBUILT, from host and from device arrays); a plain rtx_scene_pose afterwards shows the uploaded colours."""
    torch = pytest.importorskip("torch")
    r = cs.class_render(orc, samples_seeded, ground, nb_ray, nb_light)
    prims, plain = r["prims"], cs.ordinary_prims(r["prims"])
    osc = cs.class_scene(orc, samples_seeded, plain, nb_ray, nb_light)
    uploaded, _ = osc.render_rows(mode=orc.MODE_BVH)
    osc.close()
    assert (uploaded != r["frame"]).any()
    tally = Tally("posed classes, ground %s, nb_ray %d, %d samples" % (ground, nb_ray, nb_light))
    camera = vs.camera(cs.CLASS_VIEW)
    view = lib_view(rtx, cs.CLASS_FRAME, camera)
    o, d = primary_rays(orc, cs.CLASS_FRAME, camera, samples_seeded, nb_ray)
    given = dict(v0v1v2=None, spheres=None, rgb=prims["rgb"], sphere_rgb=prims["sphere_rgb"])
    kw, keep = on_device(torch, dict(given, v0v1v2=prims["tris"]))
    stream = torch.cuda.current_stream().cuda_stream
    with cs.class_scene(rtx, samples_seeded, plain, nb_ray, nb_light, frame=(8, 8), reference_tree=rtx.REFTREE_NEVER, tie_rank=None) as scene:
        for rebuilt in (False, True):
            for variant in ("host", "device"):
                what = "%s, %s variant" % ("rebuilt" if rebuilt else "refitted", variant)
                if variant == "host":
                    scene.pose_prims(rebuilt=rebuilt, **given)
                else:
                    scene.pose_prims_device(0, rebuilt=rebuilt, stream=stream, **kw)
                posed_frame(tally, scene, view, r["frame"], r["lin"], what, nan=True)
                shaded(tally, scene, o, d, r["frame"], r["lin"], hit_counts(r), what, posed=True)
            (scene.pose_rebuilt if rebuilt else scene.pose)(prims["tris"])
            tally.same(scene.render_view_rows(view, posed=True), uploaded, "a plain pose afterwards: rows")
            tally.same(scene.render_view(view, posed=True), uploaded, "a plain pose afterwards: view")
        tally.same(scene.render_view_rows(view), uploaded, "the unposed rows")
        torch.cuda.synchronize()
    tally.check()


def test_class_colours_under_a_given_light(rtx, orc, samples_seeded):
    tri, count = ls.SIDE_LIGHTS["far_side"]
    r = cs.class_render(orc, samples_seeded, "ordinary", 2, count, light_tri=tri)
    own = cs.class_render(orc, samples_seeded, "ordinary", 2, 4)
    assert (r["frame"] != own["frame"]).any()
    tally = Tally("classes under the far-side light")
    view = lib_view(rtx, cs.CLASS_FRAME, vs.camera(cs.CLASS_VIEW))
    light = rtx.Scene.make_light(tri, count)
    with cs.class_scene(rtx, samples_seeded, r["prims"], 2, 4, reference_tree=rtx.REFTREE_NEVER, tie_rank=None) as scene:
        tally.same(scene.render_view_rows(view, light=light), r["frame"], "lit view rows")
        tally.same(scene.render_view_rows(view), own["frame"], "the scene's own light afterwards")
    tally.check()


def test_ladder_values_beside_a_huge_neighbour(rtx, orc, samples_seeded):
    """An ordinary grey quad's pixel at 16 gamma steps and one float below, in the grey tile whose 2^61 members send their
    wavefronts to the true division: the in-range lanes' quotients must be the ones the short steps give."""
    nb_ray, nb_light = cs.CLASS_LADDER_CONFIG
    entries = cs.class_ladder(orc, samples_seeded)
    base = cs.class_prims(orc, samples_seeded)
    tally = Tally("class ladder, %d colours" % len(entries))
    view = lib_view(rtx, cs.CLASS_FRAME, vs.camera(cs.CLASS_VIEW))
    with cs.class_scene(rtx, samples_seeded, base, nb_ray, nb_light, reference_tree=rtx.REFTREE_NEVER, tie_rank=None) as scene:
        for what, rgb, e in entries:
            r = cs.class_render(orc, samples_seeded, "ordinary", nb_ray, nb_light, ladder_rgb=tuple(rgb))
            scene.pose_prims(rgb=r["prims"]["rgb"])
            posed_frame(tally, scene, view, r["frame"], r["lin"], what, nan=True)
            if e["step"] % 2:
                with cs.class_scene(rtx, samples_seeded, r["prims"], nb_ray, nb_light, reference_tree=rtx.REFTREE_NEVER, tie_rank=None) as fresh:
                    tally.same(gf.render_both(fresh)[0], r["frame"], what + ": rows of a fresh scene")
    tally.check()


@pytest.mark.parametrize("ground", list(cs.WHOLE_GROUNDS))
def test_the_whole_stream_form_with_class_colours(rtx, orc, samples_seeded, ground):
    """shade_tiles_kernel<.., WHOLE = true>: the true division and registers of its own"""
    w = cs.whole_stream(orc, rtx, samples_seeded, ground)
    tally = Tally("whole stream, ground %s" % ground)
    with rtx.Scene(cs.WHOLE_FRAME[0], cs.WHOLE_FRAME[1], w["tris"], w["rgb"], samples_seeded, nb_ray=cs.WHOLE_NB_RAY,
                   nb_light_sample=cs.WHOLE_LIGHT, leaf_max=1, reference_tree=rtx.REFTREE_NEVER, tie_rank=None, **w["extra"]) as scene:
        info = scene.info()
        assert info["n_nodes"] > gf.CUT_MAX_NODES and info["n_ref_nodes"] == 0, info
        img, st = gf.render_both(scene)
        assert st["primary_hits"] == w["stats"]["primary_hits"] and st["redo_tiles"] == 0, st
        tally.same(img, w["frame"], "rows")
    tally.check()
