"""GPU parity of rtx_render_view_rows_shade (and its device-resident variant): the render pipeline's RtxPixelShade records
against rtx_render_view_lit's / rtx_render_view_posed's records for the same view and light (accum_sets.same_records: the
linear words bit for bit, a NaN standing for any NaN, the bytes, the hit counts), against the oracle's frames and linear
colours where a fixture holds them, and the records' bytes against rtx_render_view_rows*'s.  The tolerance is zero
throughout.

Every frame here is far smaller than the shading pass's grid (24 tiles or fewer against 256 workgroups and more), so the
costliest class of every launch lies above order_tiles_kernel's split limit — limit <= total / grid, while the costliest
tile costs at least total / scheduled tiles — and its tiles are cut into parts: the record form's `mine` rule (a pixel is
stored by the part that holds its hit record, a pixel without one by part 0) is exercised by every test below."""
import ctypes as C
import importlib
import os

import numpy as np
import pytest

import accum_sets as ac
import colour_sets as cs
import gpu_forms as gf
import light_sets as ls
import lit_rows_sets as lr
import posed_rows_sets as pr
import prims_sets as pm
import view_rows_sets as vr
import view_sets as vs
from query_sets import H, W

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUNNY = os.path.join(ROOT, "models", "big_bunny.obj")
GUARD = 0xA5


@pytest.fixture(scope="module")
def rtx():
    mod = importlib.import_module("ray-tracer-rust_amd")
    assert mod.device_count() >= 1, "no HIP device: the product path has no CPU fallback"
    return mod


@pytest.fixture(scope="module")
def bunny(rtx, samples_seeded):
    scene = rtx.default_scene([BUNNY], W, H, samples_seeded)
    yield scene
    scene.close()


def lib_view(rtx, v, rows=None):
    (w, h) = v[0]
    return rtx.Scene.view(w, h, rect=None if rows is None else (0, rows[0], w, rows[1]), **vs.camera(v))


def check_records(scene, view, what, light=None, posed=False, frame=None, lin=None):
    """the pipeline's records, counted and uncounted, against the view kernel's for the same view and light, their bytes
    against the byte launch's and — where the fixture has them — the oracle's frame and linear colours -> the records"""
    got, st = scene.render_view_rows_shade(view, stats=True, light=light, posed=posed)
    rgb, want, vst = scene.render_view(view, want_shade=True, stats=True, light=light, posed=posed)
    assert got.shape == want.shape == (view.ny, view.width)
    bad = np.argwhere((ac.qs.bits(got["linear"]) != ac.qs.bits(want["linear"])).any(axis=2) | (got["hits"] != want["hits"]))
    assert ac.same_records(got, want), "%s: records differ from the view kernel's, first (y, x) %s" % (what, bad[:6].tolist())
    assert ac.same_records(scene.render_view_rows_shade(view, light=light, posed=posed), got), what + ": counted and uncounted"
    rows = scene.render_view_rows(view, light=light, posed=posed)
    assert np.array_equal(got["rgb8"], rows) and np.array_equal(rows, rgb), what + ": the records' bytes and the byte launch's"
    for k in ("primary_rays", "primary_hits", "shadow_rays", "rays"):
        assert st[k] == vst[k], (what, k, st[k], vst[k])
    if frame is not None:
        assert np.array_equal(got["rgb8"], frame), what + ": bytes differ from the oracle's frame"
    if lin is not None:
        nan = np.isnan(lin)
        assert np.array_equal(np.isnan(got["linear"]), nan) and np.array_equal(ac.qs.bits(got["linear"])[~nan], ac.qs.bits(lin)[~nan]), \
            what + ": linear words differ from the oracle's"
    return got


# ---------------------------------------------------------------------------------------------- 1: bunny + ground
@pytest.mark.parametrize("name", ["far_side", "grazing"])
def test_side_view_under_another_light(rtx, orc, samples_seeded, bunny, name):
    fx = lr.side(orc, samples_seeded, name)
    got = check_records(bunny, lib_view(rtx, fx["v"]), name, light=rtx.Scene.make_light(fx["light"], fx["count"]), frame=fx["frame"])
    assert (got["hits"] == 0).sum() >= 10 and (got["hits"] == 1).sum() >= 10


@pytest.mark.parametrize("count", [1, 100, 129])
def test_own_triangle_at_other_counts(rtx, orc, samples_seeded, bunny, count):
    fx = lr.own(orc, samples_seeded, count)
    check_records(bunny, lib_view(rtx, fx["v"]), "count %d" % count, light=rtx.Scene.make_light(fx["light"], fx["count"]),
                  frame=fx["frame"])


def test_own_light_and_the_turntable(rtx, orc, samples_seeded, bunny):
    check_records(bunny, lib_view(rtx, lr.SIDE), "side, own light")
    for k, fx in enumerate(lr.orbit(orc, samples_seeded)[:2]):
        check_records(bunny, lib_view(rtx, fx["v"]), "orbit %d" % k, light=rtx.Scene.make_light(fx["light"], fx["count"]),
                      frame=fx["frame"])
    assert np.array_equal(bunny.render_view_rows_shade(bunny.own_view())["rgb8"], bunny.render_rows())


# ---------------------------------------------------------------------------------------------- 2: two rays, spheres, poses
def test_yard_two_rays_per_pixel_unposed_and_posed(rtx, orc, samples_seeded):
    """the hit counts a launch's passes hand on (RecordOut::hits) beside the sums (StreamWorkspace::acc): pixels with 0, 1 and
    2 of their two rays hit, from accum_sets' low eye, where the spheres and the mesh stand against the sky"""
    view = ac.yard_view(rtx)
    with pm.open_yard(rtx, samples_seeded) as yard:
        got = check_records(yard, view, "yard")
        assert all((got["hits"] == n).sum() >= 10 for n in (0, 1, 2)), np.bincount(got["hits"].ravel())
        check_records(yard, view, "yard, another light", light=rtx.Scene.make_light(*pm.POSE_LIGHT))
        for name in ("all", "identity"):
            yard.pose_prims(**pm.given(rtx, name))
            posed = check_records(yard, view, "yard posed " + name, posed=True)
            assert ac.same_records(posed, got) == (name == "identity")
            check_records(yard, view, "yard posed %s, another light" % name, posed=True, light=rtx.Scene.make_light(*pm.POSE_LIGHT))
        assert ac.same_records(yard.render_view_rows_shade(view), got), "the unposed records after the poses"


def test_lifted_ground(rtx, orc, samples_seeded):
    fx = pr.lifted(orc, samples_seeded)
    with pr.lift_scene(rtx, samples_seeded) as scene:
        view = lib_view(rtx, pr.LIFT_VIEW)
        check_records(scene, view, "before the pose", frame=fx["still"])
        scene.pose(pr.lift_pose())
        check_records(scene, view, "lifted", posed=True, frame=fx["frame"])
        check_records(scene, view, "unposed after the pose", frame=fx["still"])


# ---------------------------------------------------------------------------------------------- 3: colours out of range
@pytest.mark.parametrize("nb_ray,nb_light", cs.CLASS_CONFIGS)
@pytest.mark.parametrize("ground", list(cs.GROUND_VARIANTS))
def test_class_colours(rtx, orc, samples_seeded, ground, nb_ray, nb_light):
    """colour_sets' 16 classes (negative, NaN, infinite, subnormal, huge colours; grey and coloured tiles): the grey-tile
    contributions, the open-ground loop and div_denom's short steps against the view kernel's division, word for word"""
    r = cs.class_render(orc, samples_seeded, ground, nb_ray, nb_light)
    view = lib_view(rtx, cs.CLASS_VIEW)
    with cs.class_scene(rtx, samples_seeded, r["prims"], nb_ray, nb_light, reference_tree=rtx.REFTREE_NEVER, tie_rank=None) as scene:
        check_records(scene, view, "classes", frame=r["frame"], lin=r["lin"])


# ---------------------------------------------------------------------------------------------- 4: the reference re-render
@pytest.mark.parametrize("name", ["P", "S"])
def test_hard_primary_rays_reach_the_reference_kernels_record_form(rtx, orc, samples_seeded, name):
    """view_sets' hard-ray scenes through their descriptions' own axis cameras: P's -0.0 primary direction components queue
    tiles in the SCHEDULING pass (S, the same camera over spheres, has none); reference_records_kernel re-renders them and
    counts the hits itself"""
    hs = vs.hard_scene(name, orc, samples_seeded, rtx)
    hard_tiles, _ = vs.neg_zero_tiles(hs["ref"])
    with rtx.Scene(*hs["args"], **hs["kw"]) as scene:
        view = lib_view(rtx, hs["v"])
        _, st = scene.render_view_rows_shade(view, stats=True)
        assert (st["redo_tiles"] > 0) == (hard_tiles > 0) == (name == "P"), (name, st["redo_tiles"], hard_tiles)
        check_records(scene, view, name, frame=hs["ref"]["frame"])
        check_records(scene, view, name + " under another light", light=rtx.Scene.make_light((5.0, 11.0, -2.0, 8.0, 11.0, -2.0, 6.0, 12.0, 2.0), 9))


def test_hard_shadow_directions_reach_it_through_the_shading_pass(rtx, orc, samples_seeded, bunny):
    """a light whose points overflow (lit_rows_sets.OVERFLOW_LIGHTS): every shadow direction is inf / inf = NaN, a hard
    direction, which only a job of the SHADING pass meets — the side view queues no tile under an ordinary light — so
    every tile with a hit is re-rendered by reference_records_kernel"""
    view = lib_view(rtx, lr.SIDE)
    _, plain = bunny.render_view_rows_shade(view, stats=True)
    assert plain["redo_tiles"] == 0
    for tri in lr.OVERFLOW_LIGHTS[:2]:
        light = rtx.Scene.make_light(tri, 7)
        _, st = bunny.render_view_rows_shade(view, stats=True, light=light)
        with_a_hit = int((bunny.tile_descs()[:, 1] > 0).sum())
        assert st["redo_tiles"] == with_a_hit > 0, (st["redo_tiles"], with_a_hit)
        got = check_records(bunny, view, "overflowing light", light=light)
        assert (got["hits"] == 1).sum() >= 10


# ---------------------------------------------------------------------------------------------- 5: other forms
@pytest.mark.parametrize("n_spheres", [0, 40])
def test_whole_stream_form(rtx, samples_seeded, n_spheres):
    tris, rgb, extra = gf.whole_stream_scene(rtx, n_spheres=n_spheres)
    with rtx.Scene(24, 24, tris, rgb, samples_seeded, nb_ray=2, nb_light_sample=4, leaf_max=1, reference_tree=rtx.REFTREE_NEVER,
                   tie_rank=None, **extra) as scene:
        assert scene.info()["n_nodes"] > gf.CUT_MAX_NODES
        got = check_records(scene, scene.own_view(), "whole stream, %d spheres" % n_spheres)
        assert got["hits"].max() == 2 and np.array_equal(got["rgb8"], scene.render_rows())
        check_records(scene, lib_view(rtx, ((21, 13), (150.0, 160.0, 170.0), (-15.0, 100.0, 0.0), 16.0)), "whole stream, another view",
                      light=rtx.Scene.make_light((-40.0, 290.0, 60.0, -10.0, 290.0, 60.0, -25.0, 300.0, 90.0), 6))


def test_a_scene_that_aims_nothing(rtx, samples_half):
    scene, _ = vr.make_scene(rtx, "one_triangle", samples_half[:64])
    with scene:
        assert not scene.primary_nodes()[1]
        v = rtx.Scene.view(19, 11, eye=(0.5, 1.0, 6.0), look_at=(1.0, 1.0, -3.0), distance=15.0)
        got = check_records(scene, v, "one triangle", light=rtx.Scene.make_light((3.0, 4.0, 2.0, 4.0, 4.0, 2.0, 3.5, 5.0, 3.0), 130))
        assert got["hits"].any()


# ---------------------------------------------------------------------------------------------- 6: row windows, guards
def test_row_windows_off_the_tile_grid_and_a_width_off_it(rtx, orc, samples_seeded, bunny):
    torch = pytest.importorskip("torch")
    fx = lr.side(orc, samples_seeded, "far_side")
    light = rtx.Scene.make_light(fx["light"], fx["count"])
    whole = bunny.render_view(lib_view(rtx, fx["v"]), want_shade=True, light=light)[1]
    odd = ((43, 29),) + tuple(fx["v"][1:])                 # 43 pixels: five whole tiles and three columns of a sixth
    whole_odd = bunny.render_view(lib_view(rtx, odd), want_shade=True, light=light)[1]
    for v, want_all, windows in ((fx["v"], whole, ((3, 13), (8, 8), (31, 1))), (odd, whole_odd, ((3, 13), (0, 29)))):
        w = v[0][0]
        for y0, ny in windows:
            view = lib_view(rtx, v, (y0, ny))
            # host variant: 64 guard bytes on both sides
            buf = np.full(ny * w * 16 + 128, GUARD, np.uint8)
            out = buf[64:64 + ny * w * 16]
            rc = rtx.rtx._lib.rtx_render_view_rows_shade(bunny.handle, 0, C.byref(view), C.byref(light), 0,
                                                         C.cast(out.ctypes.data, C.POINTER(rtx.rtx.PixelShade)), None)
            assert rc == rtx.OK and (buf[:64] == GUARD).all() and (buf[64 + ny * w * 16:] == GUARD).all(), (w, y0, ny)
            assert ac.same_records(out.view(rtx.PIXEL_SHADE_DTYPE).reshape(ny, w), want_all[y0:y0 + ny]), (w, y0, ny)
            # device-resident variant: the kernels' own stores against 64 guard bytes on both sides
            d = torch.full((ny * w * 16 + 128,), GUARD, dtype=torch.uint8, device="cuda:0")
            assert (d.data_ptr() + 64) % 16 == 0
            s = torch.cuda.current_stream().cuda_stream
            bunny.render_view_rows_shade_device(0, view, d.data_ptr() + 64, ny * w * 16, s, light=light)
            torch.cuda.synchronize()
            h = d.cpu().numpy()
            assert (h[:64] == GUARD).all() and (h[64 + ny * w * 16:] == GUARD).all(), (w, y0, ny)
            assert ac.same_records(h[64:64 + ny * w * 16].view(rtx.PIXEL_SHADE_DTYPE).reshape(ny, w), want_all[y0:y0 + ny]), (w, y0, ny)
            for bad_ptr, bad_bytes in ((d.data_ptr() + 68, ny * w * 16), (d.data_ptr() + 64, ny * w * 16 - 1)):
                with pytest.raises(rtx.RtxError) as e:
                    bunny.render_view_rows_shade_device(0, view, bad_ptr, bad_bytes, s, light=light)
                assert e.value.code == rtx.ERR_BAD_ARG


# ---------------------------------------------------------------------------------------------- 7: a shrinking and growing workspace
def test_record_launches_alternate_with_byte_launches_and_rows(rtx, orc, samples_seeded):
    far = lr.side(orc, samples_seeded, "far_side")
    light = rtx.Scene.make_light(far["light"], far["count"])
    side, small = lib_view(rtx, lr.SIDE), lib_view(rtx, lr.SIDE, rows=(5, 9))
    with rtx.default_scene([BUNNY], W, H, samples_seeded) as fresh:
        want = dict(rows=fresh.render_rows(), lit=fresh.render_view(side, want_shade=True, light=light)[1],
                    own=fresh.render_view(side, want_shade=True)[1])
    with rtx.default_scene([BUNNY], W, H, samples_seeded) as scene:
        for k in range(2):
            assert ac.same_records(scene.render_view_rows_shade(side, light=light), want["lit"]), k
            assert np.array_equal(scene.render_view_rows(side, light=light), far["frame"]), k
            assert ac.same_records(scene.render_view_rows_shade(small), want["own"][5:14]), k
            assert np.array_equal(scene.render_rows(), want["rows"]), k
            assert ac.same_records(scene.render_view_rows_shade(side), want["own"]), k
            assert np.array_equal(scene.render_view_rows(small, light=light), far["frame"][5:14]), k
        sched, shade = scene.launch_timings()
        assert len(sched) == 12 and sched[-2] > 0 and shade[-2] > 0          # a record launch counts as a launch
        scene.render_view_rows_shade(side)
        assert len(scene.tile_descs()) == 64


# ---------------------------------------------------------------------------------------------- 8: device-resident
def test_two_device_resident_launches_on_a_stream_of_their_own(rtx, orc, samples_seeded, bunny):
    torch = pytest.importorskip("torch")
    fxs = [lr.side(orc, samples_seeded, n) for n in ("far_side", "grazing")]
    view = lib_view(rtx, lr.SIDE)
    n = view.ny * view.width * 16
    wants = [bunny.render_view(view, want_shade=True, stats=True, light=rtx.Scene.make_light(fx["light"], fx["count"])) for fx in fxs]
    stream = torch.cuda.Stream(device="cuda:0")
    with torch.cuda.stream(stream):
        bufs = [torch.full((n + 16,), 0xAA, dtype=torch.uint8, device="cuda:0") for _ in fxs]
        counters = torch.zeros(8, dtype=torch.int64, device="cuda:0")
        stream.synchronize()
        for fx, b in zip(fxs, bufs):
            bunny.render_view_rows_shade_device(0, view, b.data_ptr(), n, stream.cuda_stream, counters.data_ptr(),
                                                light=rtx.Scene.make_light(fx["light"], fx["count"]))
        third = lr.side(orc, samples_seeded, "point")      # a host call right behind them: it waits for the light's use
        host = bunny.render_view_rows_shade(view, light=rtx.Scene.make_light(third["light"], third["count"]))
        assert np.array_equal(host["rgb8"], third["frame"])
        stream.synchronize()
        for (rgb, want, st), b in zip(wants, bufs):
            out = b.cpu().numpy()
            assert (out[n:] == 0xAA).all() and ac.same_records(out[:n].view(rtx.PIXEL_SHADE_DTYPE).reshape(view.ny, view.width), want)
        assert int(counters.cpu().numpy()[0]) == sum(w[2]["primary_hits"] for w in wants)
