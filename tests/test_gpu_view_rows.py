"""GPU parity of rtx_render_view_rows (and its device-resident variant): any pinhole view of an uploaded scene through the
render pipeline, against the two expected values of tests/view_sets.py (the oracle scene created with the view's camera;
render_pixel composed from oracle pieces on the view's rays), against rtx_render_view and rtx_render_rows, and the aim
kernels' stream against its host statement (tests/view_rows_sets.py, pinned without a GPU by tests/test_view_rows_host.py).
The tolerance is zero throughout."""
import ctypes as C
import importlib
import os

import numpy as np
import pytest

import query_sets as qs
import shade_sets as ss
import view_rows_sets as vr
import view_sets as vs
from query_sets import H, NO_HIT, W

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 0xA5


@pytest.fixture(scope="module")
def rtx():
    mod = importlib.import_module("ray-tracer-rust_amd")
    assert mod.device_count() >= 1, "no HIP device: the product path has no CPU fallback"
    return mod


def fresh_bunny(rtx, samples):
    return rtx.default_scene([os.path.join(ROOT, "models", "big_bunny.obj")], W, H, samples)


@pytest.fixture(scope="module")
def bunny(rtx, orc, samples_seeded):
    """big_bunny + ground created 32 x 32 with the default camera: the scene every bunny view is rendered on"""
    sets = ss.bunny_sets(orc, samples_seeded)
    scene = fresh_bunny(rtx, samples_seeded)
    assert scene.info()["n_tris"] == 4969 and scene.info()["n_global"] == 1 and scene.primary_nodes()[1]
    yield dict(scene=scene, sets=sets)
    scene.close()


def lib_view(rtx, v, rows=None):
    (w, h) = v[0]
    return rtx.Scene.view(w, h, rect=None if rows is None else (0, rows[0], w, rows[1]), **vs.camera(v))


# ---------------------------------------------------------------------------------------------- 1: the aimed stream
@pytest.mark.parametrize("name", [n for n in vr.SCENES if n != "one_triangle"])
def test_the_aim_kernels_make_the_host_statements_stream(rtx, samples_half, name):
    scene, coords = vr.make_scene(rtx, name, samples_half[:64])
    with scene:
        assert scene.primary_nodes()[1]
        delta = vr.cull_delta(coords, vr.CREATED_EYE[name])
        for eye in vr.eyes(name, delta):
            want, got = scene.aimed_nodes(eye), scene.debug_aimed_nodes(eye)
            bad = np.argwhere(got != want)
            assert not len(bad), "%s, eye %s: %d words differ, first (record, word) %s" % (name, eye, len(bad), bad[:4].tolist())
        # the same eye again, and on a scene that has rendered: the kernels run whatever the buffer holds
        scene.render_rows()
        assert np.array_equal(scene.debug_aimed_nodes(eye), want)


def test_a_scene_without_a_primary_stream_aims_nothing_and_renders(rtx, orc, samples_half):
    """one triangle (it is global: nothing beside it) and brute force: the primary rays walk the uploaded stream"""
    T = samples_half[:64]
    scene, _ = vr.make_scene(rtx, "one_triangle", T)
    with scene:
        assert not scene.primary_nodes()[1]
        assert np.array_equal(scene.debug_aimed_nodes((3.0, 2.0, 1.0)), scene.aimed_nodes((3.0, 2.0, 1.0)))
        v = rtx.Scene.view(19, 11, eye=(0.5, 1.0, 6.0), look_at=(1.0, 1.0, -3.0), distance=15.0)
        rows, st = scene.render_view_rows(v, stats=True)
        assert np.array_equal(rows, scene.render_view(v)) and st["primary_hits"] > 0
    tris, rgb, spheres, srgb, kinds = vr.mixed_scene(np.random.default_rng(5), 120, 30)
    kw = dict(eye=(1.0, 2.0, 9.0), look_at=(0.0, 0.0, -20.0), distance=20.0, tie_rank=None, nb_light_sample=4)
    with rtx.Scene(16, 12, tris, rgb, T, spheres=spheres, sphere_rgb=srgb, kinds=kinds, accel=rtx.ACCEL_BRUTE, **kw) as brute:
        assert not brute.primary_nodes()[1]
        v = rtx.Scene.view(21, 13, eye=(-4.0, 3.0, 8.0), look_at=(0.0, 0.0, -14.0), distance=18.0)
        rows, st = brute.render_view_rows(v, stats=True)
        assert np.array_equal(rows, brute.render_view(v)) and st["primary_hits"] > 0


# ---------------------------------------------------------------------------------------------- 2: whole frames
@pytest.mark.parametrize("name", ["side", "back"])
def test_whole_frames_of_other_cameras(rtx, orc, samples_seeded, bunny, name):
    view = vs.bunny_view(orc, samples_seeded, name)
    scene, v = bunny["scene"], lib_view(rtx, view["v"])
    w, h = view["w"], view["h"]
    rgb, st = scene.render_view_rows(v, stats=True)
    assert rgb.shape == (h, w, 3)
    assert np.array_equal(rgb, view["frame"]), name + ": bytes differ from the oracle scene of that camera"
    assert np.array_equal(rgb, view["set"]["shade"]["rgb8"].reshape(h, w, 3)), name + ": bytes differ from the composition"
    assert np.array_equal(rgb, scene.render_view(v)), name + ": bytes differ from rtx_render_view's"
    assert np.array_equal(scene.render_view_rows(v), rgb), name + ": with and without stats"
    hits = view["stats"]["primary_hits"]
    assert hits == int((view["set"]["hit"]["prim"] != NO_HIT).sum())
    assert st["primary_rays"] == w * h and st["primary_hits"] == hits, (name, st)
    assert st["shadow_rays"] == orc.NB_LIGHT_SAMPLE * hits == view["stats"]["shadow_rays"], (name, st)
    assert st["rays"] == st["primary_rays"] + st["shadow_rays"] and st["redo_tiles"] == 0, (name, st)


# ---------------------------------------------------------------------------------------------- 3: the scene's own view
def test_own_view_is_render_rows(rtx, orc, bunny):
    scene = bunny["scene"]
    own = scene.own_view()
    rows, st_rows = scene.render_rows(stats=True)
    got, st = scene.render_view_rows(own, stats=True)
    assert np.array_equal(got, rows) and np.array_equal(got, bunny["sets"]["osc"].render_rows(mode=orc.MODE_BVH)[0])
    for k in ("primary_rays", "primary_hits", "shadow_rays", "rays", "redo_tiles"):
        assert st[k] == st_rows[k], (k, st, st_rows)
    own.y0, own.ny = 5, 20
    assert np.array_equal(scene.render_view_rows(own), scene.render_rows(5, 20))


# ---------------------------------------------------------------------------------------------- 4: row windows
def test_row_windows_of_side(rtx, orc, samples_seeded, bunny):
    """the frame is 44 x 27: off the 8-pixel grid both ways; not a byte changes beyond the output's end"""
    view = vs.bunny_view(orc, samples_seeded, "side")
    w, h = view["w"], view["h"]
    assert (w % 8, h % 8) == (4, 3)
    for y0, ny in ((3, 13), (8, 8), (h - 1, 1), (0, h)):
        n = ny * w * 3
        buf = np.full(n + 64, GUARD, np.uint8)
        v = lib_view(rtx, view["v"], (y0, ny))
        rc = rtx.rtx._lib.rtx_render_view_rows(bunny["scene"].handle, 0, C.byref(v), buf.ctypes.data, None)
        assert rc == rtx.OK, (y0, ny)
        assert (buf[n:] == GUARD).all(), "bytes changed beyond the output's end"
        assert np.array_equal(buf[:n].reshape(ny, w, 3), view["frame"][y0:y0 + ny]), (y0, ny)
        assert np.array_equal(view["osc"].render_window(0, y0, w, ny, mode=orc.MODE_BVH)[0], view["frame"][y0:y0 + ny])


# ---------------------------------------------------------------------------------------------- 5: hard rays
@pytest.mark.parametrize("name, hits", [("P", 2526), ("S", 1241)])
def test_hard_rays_through_another_scenes_camera(rtx, orc, samples_seeded, name, hits):
    """the scene is created 16 x 16 from somewhere else; its description's own axis camera is the view: the centre row's
    -0.0 direction components (P) send their tiles through the pipeline's reference re-render, with the view's eye"""
    hs = vs.hard_scene(name, orc, samples_seeded, rtx)
    hard_tiles, hard_rays = vs.neg_zero_tiles(hs["ref"])
    assert (hard_tiles > 0) == (name == "P")
    with rtx.Scene(*hs["args"], **hs["kw"]) as scene:
        v = lib_view(rtx, hs["v"])
        rgb, st = scene.render_view_rows(v, stats=True)
        assert np.array_equal(rgb, hs["ref"]["frame"])
        assert np.array_equal(rgb, scene.render_view(v))
        assert st["primary_hits"] == hits == int(hs["ref"]["hits"].sum())
        print("%s: redo_tiles %d, tiles holding a -0.0 primary ray %d (%d rays)" % (name, st["redo_tiles"], hard_tiles, hard_rays))
        if hard_tiles:
            assert st["redo_tiles"] > 0
        else:
            assert st["redo_tiles"] == 0
        assert np.array_equal(scene.render_view_rows(v), rgb)


# ---------------------------------------------------------------------------------------------- 6: spheres, two rays per pixel
def test_soup_view_with_spheres_and_two_rays(rtx, orc, samples_seeded):
    view = vs.soup_view(orc, samples_seeded)
    a = view["a"]
    assert vs.sphere_rays(view) >= 50
    with rtx.Scene(*a["args"], nb_ray=2, **a["kw"]) as scene:
        v = lib_view(rtx, view["v"])
        rgb, st = scene.render_view_rows(v, stats=True)
        assert np.array_equal(rgb, view["frame"]) and np.array_equal(rgb, scene.render_view(v))
        assert np.array_equal(rgb, view["set"]["shade"]["rgb8"].reshape(view["h"], view["w"], 3))
        assert st["primary_rays"] == 2 * view["w"] * view["h"] and st["primary_hits"] == view["stats"]["primary_hits"], st


# ---------------------------------------------------------------------------------------------- 7: state
def test_a_view_leaves_every_other_call_unchanged(rtx, orc, samples_seeded, bunny):
    cam = bunny["sets"]["camera"]
    side, back = (lib_view(rtx, vs.bunny_view(orc, samples_seeded, n)["v"]) for n in ("side", "back"))
    solo = {}
    with fresh_bunny(rtx, samples_seeded) as a:
        solo["side"] = a.render_view_rows(side).tobytes()
    with fresh_bunny(rtx, samples_seeded) as b:
        solo["back"] = b.render_view_rows(back).tobytes()
    with fresh_bunny(rtx, samples_seeded) as c:
        solo["rows"] = c.render_rows().tobytes()
    with fresh_bunny(rtx, samples_seeded) as d:
        solo["trace"] = d.trace_rays(cam["origins"], cam["directions"]).tobytes()
    assert solo["side"] == vs.bunny_view(orc, samples_seeded, "side")["frame"].tobytes()
    assert solo["back"] == vs.bunny_view(orc, samples_seeded, "back")["frame"].tobytes()
    with fresh_bunny(rtx, samples_seeded) as s:
        steps = [("rows", lambda: s.render_rows()), ("side", lambda: s.render_view_rows(side)), ("rows", lambda: s.render_rows()),
                 ("back", lambda: s.render_view_rows(back)), ("side", lambda: s.render_view_rows(side)),
                 ("trace", lambda: s.trace_rays(cam["origins"], cam["directions"])), ("side", lambda: s.render_view_rows(side))]
        for k, (what, call) in enumerate(steps):
            assert call().tobytes() == solo[what], "step %d (%s) differs from its solo result" % (k, what)
        assert np.array_equal(s.primary_nodes()[0], bunny["scene"].primary_nodes()[0])      # the prepared scene is not written


def test_the_workspace_shrinks_and_grows(rtx, orc, samples_seeded, bunny):
    scene = bunny["scene"]
    view = vs.bunny_view(orc, samples_seeded, "side")
    wide = lib_view(rtx, view["v"])
    small = lib_view(rtx, ((16, 16),) + tuple(view["v"][1:]))
    want_small = scene.render_view(small)
    assert want_small.any()
    for v, want in ((wide, view["frame"]), (small, want_small), (wide, view["frame"])):
        assert np.array_equal(scene.render_view_rows(v), want), (v.width, v.height)


def test_two_live_scenes_alternate_views(rtx, orc, samples_seeded, bunny):
    soup = vs.soup_view(orc, samples_seeded)
    a = soup["a"]
    side, back = (vs.bunny_view(orc, samples_seeded, n) for n in ("side", "back"))
    with rtx.Scene(*a["args"], nb_ray=2, **a["kw"]) as other:
        sv = lib_view(rtx, soup["v"])
        for view in (side, back, side, side, back):
            assert np.array_equal(bunny["scene"].render_view_rows(lib_view(rtx, view["v"])), view["frame"])
            assert np.array_equal(other.render_view_rows(sv), soup["frame"])


# ---------------------------------------------------------------------------------------------- 8: device-resident
def test_device_resident_views_back_to_back_on_a_stream_of_their_own(rtx, orc, samples_seeded, bunny):
    torch = pytest.importorskip("torch")
    assert torch.cuda.is_available(), "torch sees no GPU"
    scene = bunny["scene"]
    views = [lib_view(rtx, vs.bunny_view(orc, samples_seeded, n)["v"]) for n in ("side", "back")]
    host = [scene.render_view_rows(v, stats=True) for v in views]
    stream = torch.cuda.Stream(device="cuda:0")
    assert stream.cuda_stream != torch.cuda.default_stream().cuda_stream
    with torch.cuda.stream(stream):
        bufs = [torch.full((v.ny * v.width * 3 + 16,), 0xAA, dtype=torch.uint8, device="cuda:0") for v in views]
        counters = torch.zeros(8, dtype=torch.int64, device="cuda:0")
        stream.synchronize()
        with pytest.raises(rtx.RtxError) as e:
            scene.render_view_rows_device(0, views[0], bufs[0].data_ptr(), views[0].ny * views[0].width * 3 - 1, stream.cuda_stream)
        assert e.value.code == rtx.ERR_BAD_ARG
        for v, b in zip(views, bufs):                       # two eyes, two buffers, nothing waited for between
            scene.render_view_rows_device(0, v, b.data_ptr(), b.numel(), stream.cuda_stream, counters.data_ptr())
        stream.synchronize()
        for b, (want, _) in zip(bufs, host):
            out = b.cpu().numpy()
            assert out[:want.nbytes].tobytes() == want.tobytes()
            assert (out[want.nbytes:] == 0xAA).all()
        got = counters.cpu().numpy()
        assert int(got[0]) == host[0][1]["primary_hits"] + host[1][1]["primary_hits"], got
        # the same eye on the same stream again (no aim kernel runs), then the other one
        for k in (1, 0):
            bufs[k].fill_(0xAA)
            scene.render_view_rows_device(0, views[k], bufs[k].data_ptr(), bufs[k].numel(), stream.cuda_stream)
        stream.synchronize()
        for b, (want, _) in zip(bufs, host):
            assert b.cpu().numpy()[:want.nbytes].tobytes() == want.tobytes()
    assert np.array_equal(scene.render_view_rows(views[0]), host[0][0])                   # and back on the library's stream


# ---------------------------------------------------------------------------------------------- 9: a turntable
def test_four_turntable_eyes_on_one_scene(rtx, orc, samples_seeded, bunny):
    for v, frame, ost in vs.turntable(orc, samples_seeded):
        lv = lib_view(rtx, v)
        rgb, st = bunny["scene"].render_view_rows(lv, stats=True)
        assert rgb.shape == (16, 24, 3) and np.array_equal(rgb, frame), v[1]
        assert np.array_equal(rgb, bunny["scene"].render_view(lv)), v[1]
        assert st["primary_hits"] == ost["primary_hits"] and st["shadow_rays"] == ost["shadow_rays"], v[1]


# ---------------------------------------------------------------------------------------------- 10: launch timings
def test_a_view_launch_counts_in_the_launch_timings(rtx, orc, samples_seeded):
    view = vs.soup_view(orc, samples_seeded)
    a = view["a"]
    with rtx.Scene(*a["args"], nb_ray=2, **a["kw"]) as scene:
        scene.render_rows()
        before = len(scene.launch_timings()[0])
        assert before == 1
        scene.render_view_rows(lib_view(rtx, view["v"]))
        sched, shade = scene.launch_timings()
        assert len(sched) == len(shade) == before + 1
        assert sched[-1] > 0 and shade[-1] > 0, (sched, shade)
        import sequence_sets as sq
        assert len(scene.tile_descs()) == sq.launch_tiles(view["w"], view["h"])[1]        # rtx_debug_tile_descs: the view's launch
