"""GPU parity of rtx_render_view_rows_lit (and its device-resident variant): any view of an uploaded scene under ANOTHER
light through the render pipeline, against the expected values of tests/lit_rows_sets.py (the oracle scene created with the
view's camera and that light; render_pixel composed from oracle pieces), against rtx_render_view_lit and
rtx_render_view_rows, and the walk kernels' tour and boxes against their host statement (rtx_scene_light_walk_for, pinned
without a GPU by tests/test_lit_rows_host.py).  The tolerance is zero throughout."""
import ctypes as C
import importlib
import os

import numpy as np
import pytest

import gpu_forms as gf
import light_sets as ls
import lit_rows_sets as lr
import query_sets as qs
import sequence_sets as sq
import shade_sets as ss
import view_rows_sets as vr
import view_sets as vs
from query_sets import H, NO_HIT, W, bits

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUNNY = os.path.join(ROOT, "models", "big_bunny.obj")
GUARD = 0xA5


@pytest.fixture(scope="module")
def rtx():
    mod = importlib.import_module("ray-tracer-rust_amd")
    assert mod.device_count() >= 1, "no HIP device: the product path has no CPU fallback"
    return mod


def fresh_bunny(rtx, samples):
    return rtx.default_scene([BUNNY], W, H, samples)


@pytest.fixture(scope="module")
def bunny(rtx, samples_seeded):
    """big_bunny + ground created 32 x 32 with the default camera and light: the scene every bunny fixture is lit on"""
    scene = fresh_bunny(rtx, samples_seeded)
    assert scene.info()["n_tris"] == 4969 and scene.light().nb_light_sample == 100 and scene.primary_nodes()[1]
    yield scene
    scene.close()


def lib_view(rtx, v, rows=None):
    (w, h) = v[0]
    return rtx.Scene.view(w, h, rect=None if rows is None else (0, rows[0], w, rows[1]), **vs.camera(v))


def lib_light(rtx, fx):
    return rtx.Scene.make_light(fx["light"], fx["count"])


def check_lit_rows(rtx, scene, fx, what):
    """a whole lit frame, with and without stats, against the fixture's expected value and rtx_render_view_lit
    -> (stats, the launch's tile descriptors)"""
    view, light = lib_view(rtx, fx["v"]), lib_light(rtx, fx)
    rgb, st = scene.render_view_rows(view, stats=True, light=light)
    td = scene.tile_descs()
    assert rgb.shape == (fx["h"], fx["w"], 3)
    assert np.array_equal(rgb, fx["frame"]), "%s: bytes differ from the expected value at (y, x) %s" % (
        what, np.argwhere((rgb != fx["frame"]).any(axis=2))[:8].tolist())
    assert np.array_equal(scene.render_view_rows(view, light=light), rgb), what + ": with and without stats"
    assert np.array_equal(scene.render_view(view, light=light), rgb), what + ": bytes differ from rtx_render_view_lit's"
    hits = fx["stats"]["primary_hits"] if fx["stats"] is not None else int((fx["set"]["hit"]["prim"] != NO_HIT).sum())
    count = fx["count"] or scene.light().nb_light_sample
    assert st["primary_rays"] == fx["w"] * fx["h"] * fx["nb_ray"] and st["primary_hits"] == hits, (what, st)
    assert st["shadow_rays"] == count * hits and st["rays"] == st["primary_rays"] + st["shadow_rays"], (what, st)
    if fx["stats"] is not None:
        assert st["shadow_rays"] == fx["stats"]["shadow_rays"], what
    return st, td


# ---------------------------------------------------------------------------------------------- 1: the walk kernels
def check_walk(scene, light, what, points_are_finite=True):
    nb_ray = scene.nb_ray
    pts = scene.light_points_for(light)
    count = len(pts) // nb_ray
    order, boxes, _ = scene.light_walk_for(light)
    tour, dev_boxes = scene.debug_light_walk(light)
    want = lr.tour_records(pts, order, nb_ray, count)
    assert tour.shape == want.shape == (nb_ray * count, 4), what
    if points_are_finite:
        bad = np.argwhere(tour != want)
        assert not len(bad), "%s: %d words of the tour differ, first (record, word) %s" % (what, len(bad), bad[:4].tolist())
        assert np.array_equal(dev_boxes, boxes), (what, dev_boxes, boxes)                      # by value
    else:                                          # (a NaN's bits are its maker's: the order alone)
        assert np.array_equal(tour[:, 3], want[:, 3]), what


def test_the_walk_kernels_make_the_host_statements_walk(rtx, orc, samples_seeded, bunny):
    a = qs.scene_a(orc, samples_seeded)
    with rtx.default_scene([BUNNY], W, H, samples_seeded[:ls.WRAP_PAIRS], reference_tree=rtx.REFTREE_NEVER, tie_rank=None) as short, \
            rtx.Scene(*a["args"], nb_ray=2, **a["kw"]) as soup:
        for sname, scene in (("bunny", bunny), ("soup", soup), ("short", short)):
            for tri, lname in lr.all_lights(orc):
                for count in lr.COUNTS + ((ls.WRAP_COUNT,) if sname == "short" else ()):
                    check_walk(scene, rtx.Scene.make_light(tri, count), (sname, lname, count))
            zero = scene.light()
            zero.nb_light_sample = 0
            check_walk(scene, zero, (sname, "count 0"))
        check_walk(bunny, rtx.Scene.make_light((0.0,) * 9, 130), "every point the origin")
        for tri in lr.OVERFLOW_LIGHTS:
            for count in (7, 130):
                check_walk(bunny, rtx.Scene.make_light(tri, count), ("overflow", count), points_are_finite=False)
        # a large light after small ones (the buffers grow), and a small one again
        check_walk(bunny, rtx.Scene.make_light(ls.SIDE_LIGHTS["grazing"][0], 5001), "5001 samples")
        check_walk(bunny, rtx.Scene.make_light(ls.SIDE_LIGHTS["grazing"][0], 3), "3 samples")


# ---------------------------------------------------------------------------------------------- 2: lit frames
@pytest.mark.parametrize("name", list(ls.SIDE_LIGHTS))
def test_side_under_another_light(rtx, orc, samples_seeded, bunny, name):
    fx = lr.side(orc, samples_seeded, name)
    st, td = check_lit_rows(rtx, bunny, fx, name)
    assert len(td) == sq.launch_tiles(fx["w"], fx["h"])[1]
    finished, cut = lr.tile_classes(td, fx["w"], fx["h"])
    print("%s: %d tiles finished by the scheduling pass, %d with a cut, redo_tiles %d" % (name, finished, cut, st["redo_tiles"]))
    assert finished >= 1 and cut >= 1, "%s: the fixture does not exercise the shaft under this light" % name


@pytest.mark.parametrize("count", lr.COUNTS)
def test_own_triangle_with_another_count(rtx, orc, samples_seeded, bunny, count):
    check_lit_rows(rtx, bunny, lr.own(orc, samples_seeded, count), "count %d" % count)


def test_sample_table_shorter_than_the_count(rtx, orc, samples_seeded):
    fx = lr.wrap(orc, samples_seeded)
    with rtx.default_scene([BUNNY], W, H, fx["samples"]) as scene:
        assert len(scene.samples) == ls.WRAP_PAIRS < fx["count"]
        check_lit_rows(rtx, scene, fx, "wrap")


# ---------------------------------------------------------------------------------------------- 3: the scene's own light
def test_own_light_is_the_unlit_call(rtx, orc, samples_seeded, bunny):
    own, zero = bunny.light(), bunny.light()
    zero.nb_light_sample = 0
    for v in (bunny.own_view(), lib_view(rtx, lr.SIDE), lib_view(rtx, lr.SIDE, rows=(5, 13))):
        unlit, ust = bunny.render_view_rows(v, stats=True)
        for light in (own, zero):
            lit, st = bunny.render_view_rows(v, stats=True, light=light)
            assert lit.tobytes() == unlit.tobytes()
            for k in ("primary_rays", "primary_hits", "shadow_rays", "rays", "redo_tiles"):
                assert st[k] == ust[k], k
    assert np.array_equal(bunny.render_view_rows(bunny.own_view(), light=own), bunny.render_rows())
    # a scene without light samples, a light without a count: no light kernel runs, the bytes are the unlit call's
    with rtx.default_scene([BUNNY], W, H, samples_seeded, nb_light_sample=0, reference_tree=rtx.REFTREE_NEVER, tie_rank=None) as dark:
        v = lib_view(rtx, lr.SIDE)
        lit, st = dark.render_view_rows(v, stats=True, light=rtx.Scene.make_light(ls.SIDE_LIGHTS["far_side"][0], 0))
        assert lit.tobytes() == dark.render_view_rows(v).tobytes() and st["shadow_rays"] == 0 and st["primary_hits"] > 0
        seven = dark.render_view_rows(v, light=rtx.Scene.make_light(ls.SIDE_LIGHTS["far_side"][0], 7))
        assert np.array_equal(seven, dark.render_view(v, light=rtx.Scene.make_light(ls.SIDE_LIGHTS["far_side"][0], 7))) and seven.any()


# ---------------------------------------------------------------------------------------------- 4: row windows
def test_row_windows_off_the_tile_grid(rtx, orc, samples_seeded, bunny):
    fx = lr.side(orc, samples_seeded, "far_side")
    w, h = fx["w"], fx["h"]
    light = lib_light(rtx, fx)
    for y0, ny in ((3, 13), (8, 8), (h - 1, 1), (5, 22), (0, h)):
        n = ny * w * 3
        buf = np.full(n + 64, GUARD, np.uint8)
        v = lib_view(rtx, fx["v"], (y0, ny))
        rc = rtx.rtx._lib.rtx_render_view_rows_lit(bunny.handle, 0, C.byref(v), C.byref(light), buf.ctypes.data, None)
        assert rc == rtx.OK, (y0, ny)
        assert (buf[n:] == GUARD).all(), "bytes changed beyond the output's end"
        assert np.array_equal(buf[:n].reshape(ny, w, 3), fx["frame"][y0:y0 + ny]), (y0, ny)


# ---------------------------------------------------------------------------------------------- 5: hard rays
HARD_LIGHT = ((5.0, 11.0, -2.0, 8.0, 11.0, -2.0, 6.0, 12.0, 2.0), 9)


@pytest.mark.parametrize("name", ["P", "S"])
def test_hard_rays_under_another_light(rtx, orc, samples_seeded, name):
    """view_rows' hard-ray scenes through their descriptions' own axis cameras: the centre row's -0.0 direction components
    (P) send tiles through the reference re-render, which reads the light's points"""
    hs = vs.hard_scene(name, orc, samples_seeded, rtx)
    d = hs["ref"]["desc"]
    hard_tiles, _ = vs.neg_zero_tiles(hs["ref"])
    assert (hard_tiles > 0) == (name == "P")
    osc = orc.Scene(d["W"], d["H"], *d["args"], **dict(d["kw"], light_tri=HARD_LIGHT[0], nb_light_sample=HARD_LIGHT[1]), **d["orc_kw"])
    want, ost = osc.render_rows(mode=d["mode"])
    osc.close()
    assert not np.array_equal(want, hs["ref"]["frame"])
    with rtx.Scene(*hs["args"], **hs["kw"]) as scene:
        v, light = lib_view(rtx, hs["v"]), rtx.Scene.make_light(*HARD_LIGHT)
        rgb, st = scene.render_view_rows(v, stats=True, light=light)
        assert np.array_equal(rgb, want), name + ": bytes differ from the oracle scene created with that light"
        assert np.array_equal(rgb, scene.render_view(v, light=light)) and np.array_equal(rgb, scene.render_view_rows(v, light=light))
        assert st["primary_hits"] == ost["primary_hits"] and st["shadow_rays"] == HARD_LIGHT[1] * st["primary_hits"] == ost["shadow_rays"]
        assert (st["redo_tiles"] > 0) == (hard_tiles > 0), (name, st["redo_tiles"], hard_tiles)
        assert np.array_equal(scene.render_view_rows(v), hs["ref"]["frame"])                      # and its own light afterwards


# ---------------------------------------------------------------------------------------------- 6: spheres, two rays per pixel
def test_soup_with_spheres_and_two_rays_under_another_light(rtx, orc, samples_seeded):
    fx = lr.soup(orc, samples_seeded)
    a = fx["a"]
    with rtx.Scene(*a["args"], nb_ray=2, **a["kw"]) as scene:
        assert scene.light().nb_light_sample == 24 and ls.SOUP_LIGHT[1] == 0                    # count 0: the scene's 24
        check_lit_rows(rtx, scene, dict(fx, stats=None), "soup")
        v = lib_view(rtx, fx["v"])
        explicit = scene.render_view_rows(v, light=rtx.Scene.make_light(ls.SOUP_LIGHT[0], 24))
        assert np.array_equal(explicit, fx["frame"])


# ---------------------------------------------------------------------------------------------- 7: other forms
def test_whole_stream_scene_under_another_light(rtx, orc, samples_seeded):
    d = sq.description("Wh", orc, samples_seeded, rtx)
    light = ((-40.0, 290.0, 60.0, -10.0, 290.0, 60.0, -25.0, 300.0, 90.0), 6)
    v = ((21, 13), (150.0, 160.0, 170.0), (-15.0, 100.0, 0.0), 16.0)
    osc = orc.Scene(v[0][0], v[0][1], *d["args"], **dict(d["kw"], light_tri=light[0], nb_light_sample=light[1], **vs.camera(v)), **d["orc_kw"])
    want, ost = osc.render_rows(mode=d["mode"], nthreads=16)
    osc.close()
    with sq.make_scene(rtx, d) as scene:
        assert scene.info()["n_nodes"] > gf.CUT_MAX_NODES
        rgb, st = scene.render_view_rows(lib_view(rtx, v), stats=True, light=rtx.Scene.make_light(*light))
        assert np.array_equal(rgb, want) and want.any()
        assert st["primary_hits"] == ost["primary_hits"] and st["shadow_rays"] == light[1] * st["primary_hits"]
        assert np.array_equal(rgb, scene.render_view(lib_view(rtx, v), light=rtx.Scene.make_light(*light)))


def test_a_scene_that_aims_nothing_under_another_light(rtx, samples_half):
    scene, _ = vr.make_scene(rtx, "one_triangle", samples_half[:64])
    with scene:
        assert not scene.primary_nodes()[1]
        v = rtx.Scene.view(19, 11, eye=(0.5, 1.0, 6.0), look_at=(1.0, 1.0, -3.0), distance=15.0)
        light = rtx.Scene.make_light((3.0, 4.0, 2.0, 4.0, 4.0, 2.0, 3.5, 5.0, 3.0), 130)
        rows, st = scene.render_view_rows(v, stats=True, light=light)
        assert np.array_equal(rows, scene.render_view(v, light=light)) and st["primary_hits"] > 0
        assert st["shadow_rays"] == 130 * st["primary_hits"]


# ---------------------------------------------------------------------------------------------- 8: sequences
def test_a_sequence_of_lights_and_the_scene_afterwards(rtx, orc, samples_seeded):
    A, B = ls.SIDE_LIGHTS["far_side"][0], ls.SIDE_LIGHTS["grazing"][0]
    view = lib_view(rtx, lr.SIDE)
    cam = ss.bunny_sets(orc, samples_seeded)["camera"]
    far = lr.side(orc, samples_seeded, "far_side")
    point = rtx.Scene.make_light(*ls.SIDE_LIGHTS["point"])

    def usual(scene):
        return [scene.render_rows().tobytes(), scene.render_view_rows(view).tobytes(), scene.render_view(view, light=point).tobytes(),
                scene.shade_rays(cam["origins"], cam["directions"], force_regroup=True).tobytes()]

    with fresh_bunny(rtx, samples_seeded) as fresh:
        solo = usual(fresh)
        want = [fresh.render_view(view, light=rtx.Scene.make_light(tri, count)) for tri, count in ((A, 100), (B, 7), (A, 130))]
    assert solo[1] == lr.own(orc, samples_seeded, 100)["frame"].tobytes() and solo[3] == cam["shade"].tobytes()
    assert np.array_equal(want[0], far["frame"]) and far["count"] == 100
    with fresh_bunny(rtx, samples_seeded) as scene:
        # the workspace and the light buffers shrink and grow
        for k, (tri, count, w) in enumerate(((A, 100, 0), (B, 7, 1), (A, 130, 2), (A, 100, 0))):
            got = scene.render_view_rows(view, light=rtx.Scene.make_light(tri, count))
            assert np.array_equal(got, want[w]), "step %d" % k
        assert usual(scene) == solo
        assert np.array_equal(bits(scene.light_points()), bits(scene.light_points_for(scene.light())))


def test_two_live_scenes_alternate_lights(rtx, orc, samples_seeded, bunny):
    soup = lr.soup(orc, samples_seeded)
    a = soup["a"]
    fxs = [lr.side(orc, samples_seeded, n) for n in ("far_side", "distant")] + [lr.own(orc, samples_seeded, 7)]
    with rtx.Scene(*a["args"], nb_ray=2, **a["kw"]) as other:
        sv, sl = lib_view(rtx, soup["v"]), rtx.Scene.make_light(*ls.SOUP_LIGHT)
        for fx in (fxs[0], fxs[1], fxs[0], fxs[2], fxs[2]):
            assert np.array_equal(bunny.render_view_rows(lib_view(rtx, fx["v"]), light=lib_light(rtx, fx)), fx["frame"])
            assert np.array_equal(other.render_view_rows(sv, light=sl), soup["frame"])


# ---------------------------------------------------------------------------------------------- 9: device-resident
def test_device_resident_lit_rows_back_to_back_on_one_stream(rtx, orc, samples_seeded, bunny):
    torch = pytest.importorskip("torch")
    assert torch.cuda.is_available(), "torch sees no GPU"
    fxs = [lr.side(orc, samples_seeded, n) for n in ("far_side", "grazing")]
    view = lib_view(rtx, lr.SIDE)
    n = view.ny * view.width * 3
    stream = torch.cuda.Stream(device="cuda:0")
    assert stream.cuda_stream != torch.cuda.default_stream().cuda_stream
    with torch.cuda.stream(stream):
        bufs = [torch.full((n + 16,), 0xAA, dtype=torch.uint8, device="cuda:0") for _ in fxs]
        counters = torch.zeros(8, dtype=torch.int64, device="cuda:0")
        stream.synchronize()
        with pytest.raises(rtx.RtxError) as e:
            bunny.render_view_rows_device(0, view, bufs[0].data_ptr(), n - 1, stream.cuda_stream, light=lib_light(rtx, fxs[0]))
        assert e.value.code == rtx.ERR_BAD_ARG
        # two lights, one set of library-owned light buffers, two outputs, one counter block, nothing waited for between
        for fx, b in zip(fxs, bufs):
            bunny.render_view_rows_device(0, view, b.data_ptr(), b.numel(), stream.cuda_stream, counters.data_ptr(), light=lib_light(rtx, fx))
        # ... and a host lit view and a host lit rows call right behind them, on the library's stream: they wait for the event
        third = lr.side(orc, samples_seeded, "point")
        host_view = bunny.render_view(view, light=lib_light(rtx, third))
        host_rows = bunny.render_view_rows(view, light=lib_light(rtx, third))
        assert np.array_equal(host_view, third["frame"]) and np.array_equal(host_rows, third["frame"])
        stream.synchronize()
        for fx, b in zip(fxs, bufs):
            out = b.cpu().numpy()
            assert out[:n].tobytes() == fx["frame"].tobytes() and (out[n:] == 0xAA).all()
        got = counters.cpu().numpy()
        assert int(got[0]) == sum(fx["stats"]["primary_hits"] for fx in fxs), got


# ---------------------------------------------------------------------------------------------- 10: an orbit of lights
def test_four_lights_on_an_orbit_of_the_turntable(rtx, orc, samples_seeded, bunny):
    for k, fx in enumerate(lr.orbit(orc, samples_seeded)):
        check_lit_rows(rtx, bunny, fx, "orbit light %d" % k)


# ---------------------------------------------------------------------------------------------- 11: launch timings
def test_a_lit_launch_counts_in_the_launch_timings(rtx, orc, samples_seeded):
    fx = lr.soup(orc, samples_seeded)
    a = fx["a"]
    with rtx.Scene(*a["args"], nb_ray=2, **a["kw"]) as scene:
        scene.render_rows()
        assert len(scene.launch_timings()[0]) == 1
        scene.render_view_rows(lib_view(rtx, fx["v"]), light=rtx.Scene.make_light(*ls.SOUP_LIGHT))
        sched, shade = scene.launch_timings()
        assert len(sched) == len(shade) == 2
        assert sched[-1] > 0 and shade[-1] > 0, (sched, shade)
        assert len(scene.tile_descs()) == sq.launch_tiles(fx["w"], fx["h"])[1]
