"""GPU parity of rtx_render_view (and its device-resident variant): any pinhole view of an uploaded scene against its two
expected values (tests/view_sets.py, pinned to each other without a GPU by tests/test_view_sets.py) — the oracle scene
created with the view's camera, and render_pixel composed from oracle pieces on the scene as it is uploaded — and against
the library's own rtx_render_rows, rtx_shade_rays and rtx_trace_rays.  The tolerance is zero."""
import ctypes as C
import importlib
import os

import numpy as np
import pytest

import query_sets as qs
import shade_sets as ss
import view_sets as vs
from query_sets import H, NO_HIT, W, bits

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def rtx():
    mod = importlib.import_module("ray-tracer-rust_amd")
    assert mod.device_count() >= 1, "no HIP device: the product path has no CPU fallback"
    return mod


@pytest.fixture(scope="module")
def bunny(rtx, orc, samples_seeded):
    """big_bunny + ground created 32 x 32 with the default camera: the scene every bunny view is rendered on"""
    sets = ss.bunny_sets(orc, samples_seeded)
    scene = rtx.default_scene([os.path.join(ROOT, "models", "big_bunny.obj")], W, H, samples_seeded)
    assert scene.info()["n_tris"] == 4969 and scene.info()["n_ref_nodes"] != 0
    yield dict(scene=scene, sets=sets)
    scene.close()


def lib_view(rtx, v, rect=None):
    return rtx.Scene.view(v[0][0], v[0][1], rect=rect, **vs.camera(v))


def check_view(scene, got, view, what):
    """(rgb, shade, hits, stats) of a whole view against both expected values and the library's ray-batch calls"""
    rgb, shade, hits, st = got
    s, w, h, nb = view["set"], view["w"], view["h"], view["nb_ray"]
    assert np.array_equal(rgb, view["frame"]), what + ": bytes differ from the oracle scene of that camera"
    exp = s["shade"].reshape(h, w)
    bad = np.argwhere((bits(shade["linear"]) != bits(exp["linear"])).any(axis=2))
    assert not len(bad), "%s: linear differs at (y, x) %s" % (what, bad[:8].tolist())
    assert np.array_equal(shade["rgb8"], rgb) and np.array_equal(shade["hits"], exp["hits"]), what
    by_rays = scene.shade_rays(s["origins"], s["directions"], keep_order=True, want_hits=True)
    assert shade.tobytes() == by_rays[0].tobytes(), what + ": out_shade is not rtx_shade_rays'"
    assert hits.tobytes() == by_rays[1].tobytes(), what + ": out_hits is not rtx_shade_rays'"
    assert np.array_equal(hits["prim"].reshape(-1), s["hit"]["prim"]), what
    n_hits = int((s["hit"]["prim"] != NO_HIT).sum())
    assert st["primary_rays"] == w * h * nb and st["primary_hits"] == n_hits == view["stats"]["primary_hits"], (what, st)
    assert st["shadow_rays"] == view["stats"]["shadow_rays"] and st["rays"] == st["primary_rays"] + st["shadow_rays"], (what, st)


# ---------------------------------------------------------------------------------------------- 1: the scene's own camera
def test_own_camera(rtx, orc, bunny):
    scene, cam = bunny["scene"], bunny["sets"]["camera"]
    own = scene.own_view()
    assert (own.width, own.height, own.nx, own.ny) == (W, H, W, H)
    rgb, shade, hits, st = scene.render_view(own, stats=True, want_shade=True, want_hits=True)
    assert np.array_equal(rgb, scene.render_rows())
    assert np.array_equal(rgb, bunny["sets"]["osc"].render_rows(mode=orc.MODE_BVH)[0])
    assert shade.tobytes() == cam["shade"].tobytes()
    assert hits.tobytes() == scene.trace_rays(cam["origins"], cam["directions"], keep_order=True).tobytes()
    assert st["primary_rays"] == W * H and st["primary_hits"] == int((cam["hit"]["prim"] != NO_HIT).sum())
    plain = scene.render_view(own, want_shade=True, want_hits=True)
    assert [x.tobytes() for x in plain] == [rgb.tobytes(), shade.tobytes(), hits.tobytes()]       # with and without stats
    assert np.array_equal(scene.render_view(own), rgb)                                            # out_rgb alone
    assert scene.render_view(own, want_shade=True)[1].tobytes() == shade.tobytes()


# ---------------------------------------------------------------------------------------------- 2: other cameras
@pytest.mark.parametrize("name", ["side", "back", "far"])
def test_other_cameras(rtx, orc, samples_seeded, bunny, name):
    view = vs.bunny_view(orc, samples_seeded, name)
    got = bunny["scene"].render_view(lib_view(rtx, view["v"]), stats=True, want_shade=True, want_hits=True)
    check_view(bunny["scene"], got, view, name)


def test_far_after_side_on_one_scene(rtx, orc, samples_seeded, bunny):
    """a view from beyond the scene's bound (exact box test) right behind one from inside it (multiply-based test)"""
    scene = bunny["scene"]
    side, far = (vs.bunny_view(orc, samples_seeded, n) for n in ("side", "far"))
    alone = scene.render_view(lib_view(rtx, far["v"]), want_shade=True, want_hits=True)
    assert np.array_equal(scene.render_view(lib_view(rtx, side["v"])), side["frame"])
    after = scene.render_view(lib_view(rtx, far["v"]), want_shade=True, want_hits=True)
    assert [x.tobytes() for x in after] == [x.tobytes() for x in alone]
    assert np.array_equal(after[0], far["frame"])


# ---------------------------------------------------------------------------------------------- 3: rectangles
@pytest.mark.parametrize("rect", vs.SIDE_RECTS)
def test_rectangles_of_side(rtx, orc, samples_seeded, bunny, rect):
    """each equals the slice of the whole view and the oracle's window; not a byte changes beyond the outputs' ends"""
    view = vs.bunny_view(orc, samples_seeded, "side")
    x0, y0, nx, ny = rect
    frame, shade, hit = vs.window(view, rect)
    assert np.array_equal(view["osc"].render_window(x0, y0, nx, ny, mode=orc.MODE_BVH)[0], frame)
    L, R = rtx.rtx._lib, rtx.rtx
    n, pad = nx * ny, 64
    rgb = np.full(n * 3 + pad, 0xA5, np.uint8)
    sh = np.full(n * 16 + pad, 0xA5, np.uint8)
    hi = np.full(n * 32 + pad, 0xA5, np.uint8)
    v = lib_view(rtx, view["v"], rect)
    rc = L.rtx_render_view(bunny["scene"].handle, 0, C.byref(v), rgb.ctypes.data, sh.ctypes.data_as(C.POINTER(R.PixelShade)),
                           hi.ctypes.data_as(C.POINTER(R.RayHit)), None)
    assert rc == rtx.OK
    for buf, size in ((rgb, n * 3), (sh, n * 16), (hi, n * 32)):
        assert (buf[size:] == 0xA5).all(), "bytes changed beyond the output's end"
    assert np.array_equal(rgb[:n * 3].reshape(ny, nx, 3), frame)
    got_shade = sh[:n * 16].view(R.PIXEL_SHADE_DTYPE).reshape(ny, nx)
    assert got_shade.tobytes() == np.ascontiguousarray(shade).tobytes()
    got_hits = hi[:n * 32].view(R.RAY_HIT_DTYPE).reshape(ny, nx, 1)
    assert np.array_equal(got_hits["prim"], hit["prim"]) and np.array_equal(bits(got_hits["t"]), bits(hit["t"]))
    assert np.array_equal(bits(got_hits["p_hit"]), bits(np.ascontiguousarray(hit["p_hit"])))
    # ... and the slice of the library's own whole view, hit records included
    whole = bunny["scene"].render_view(lib_view(rtx, view["v"]), want_shade=True, want_hits=True)
    ys, xs = slice(y0, y0 + ny), slice(x0, x0 + nx)
    assert np.array_equal(rgb[:n * 3].reshape(ny, nx, 3), whole[0][ys, xs])
    assert got_shade.tobytes() == np.ascontiguousarray(whole[1][ys, xs]).tobytes()
    assert got_hits.tobytes() == np.ascontiguousarray(whole[2][ys, xs]).tobytes()


# ---------------------------------------------------------------------------------------------- 4: hard rays
@pytest.mark.parametrize("name, hits", [("P", 2526), ("S", 1241)])
def test_hard_rays_through_another_scenes_camera(rtx, orc, samples_seeded, name, hits):
    """the scene is created 16 x 16 from somewhere else; its description's own axis camera is the view: the centre row's
    -0.0 direction components (P) go through the reference walk, tile by tile"""
    hs = vs.hard_scene(name, orc, samples_seeded, rtx)
    with rtx.Scene(*hs["args"], **hs["kw"]) as scene:
        assert (scene.width, scene.height) == (16, 16)
        rgb, st = scene.render_view(lib_view(rtx, hs["v"]), stats=True)
        assert np.array_equal(rgb, hs["ref"]["frame"])
        assert st["primary_hits"] == hits == int(hs["ref"]["hits"].sum())
        if name == "P":
            assert st["redo_tiles"] > 0
        assert np.array_equal(scene.render_view(lib_view(rtx, hs["v"])), rgb)


# ---------------------------------------------------------------------------------------------- 5: the soup, two rays per pixel
def test_soup_view_with_spheres_and_two_rays(rtx, orc, samples_seeded):
    view = vs.soup_view(orc, samples_seeded)
    a = view["a"]
    with rtx.Scene(*a["args"], nb_ray=2, **a["kw"]) as scene:
        got = scene.render_view(lib_view(rtx, view["v"]), stats=True, want_shade=True, want_hits=True)
        assert got[2].shape == (22, 29, 2)
        check_view(scene, got, view, "soup")
        qs.check_normals(got[2].reshape(-1), view["set"]["hit"], scene.normals(), a["kinds"], "soup view")


# ---------------------------------------------------------------------------------------------- 6: state
def test_a_view_leaves_every_other_call_unchanged(rtx, orc, samples_seeded, bunny):
    cam = bunny["sets"]["camera"]
    side = vs.bunny_view(orc, samples_seeded, "side")
    v = lib_view(rtx, side["v"])

    def view(scene):
        return [x.tobytes() for x in scene.render_view(v, want_shade=True, want_hits=True)]

    def others(scene):
        shade, hits = scene.shade_rays(cam["origins"], cam["directions"], want_hits=True, force_regroup=True)
        return [scene.render_rows().tobytes(), shade.tobytes(), hits.tobytes(),
                scene.trace_rays(cam["origins"], cam["directions"]).tobytes()]

    def fresh():
        return rtx.default_scene([os.path.join(ROOT, "models", "big_bunny.obj")], W, H, samples_seeded)

    with fresh() as a:
        solo_view = view(a)
    with fresh() as b:
        solo_others = others(b)
    with fresh() as c:
        assert view(c) == solo_view
        assert others(c) == solo_others
        assert view(c) == solo_view
    assert solo_view[0] == side["frame"].tobytes() and solo_others[1] == cam["shade"].tobytes()


# ---------------------------------------------------------------------------------------------- 7: device-resident
def test_device_resident_views_back_to_back_on_a_stream_of_their_own(rtx, orc, samples_seeded, bunny):
    torch = pytest.importorskip("torch")
    assert torch.cuda.is_available(), "torch sees no GPU"
    scene = bunny["scene"]
    views = [lib_view(rtx, vs.bunny_view(orc, samples_seeded, n)["v"]) for n in ("side", "back")]
    host = [scene.render_view(v, want_shade=True, want_hits=True) for v in views]
    stream = torch.cuda.Stream(device="cuda:0")
    assert stream.cuda_stream != torch.cuda.default_stream().cuda_stream
    with torch.cuda.stream(stream):
        bufs = []
        for v in views:
            n = v.nx * v.ny
            bufs.append([torch.full((size + 16,), 0xAA, dtype=torch.uint8, device="cuda:0") for size in (n * 3, n * 16, n * 32)])
            assert bufs[-1][1].data_ptr() % 16 == 0 and bufs[-1][2].data_ptr() % 16 == 0
        stream.synchronize()
        with pytest.raises(rtx.RtxError) as e:
            scene.render_view_device(0, views[0], bufs[0][0].data_ptr(), bufs[0][1].data_ptr() + 8, None, stream.cuda_stream)
        assert e.value.code == rtx.ERR_BAD_ARG
        for v, b in zip(views, bufs):                       # two views, two sets of buffers, nothing waited for between
            scene.render_view_device(0, v, b[0].data_ptr(), b[1].data_ptr(), b[2].data_ptr(), stream.cuda_stream)
        stream.synchronize()
        for v, b, want in zip(views, bufs, host):
            for t, w in zip(b, want):
                out = t.cpu().numpy()
                assert out[:w.nbytes].tobytes() == w.tobytes()
                assert (out[w.nbytes:] == 0xAA).all()
        # d_rgb alone
        bufs[0][0].fill_(0xAA)
        scene.render_view_device(0, views[0], bufs[0][0].data_ptr(), None, None, stream.cuda_stream)
        stream.synchronize()
        assert bufs[0][0].cpu().numpy()[:host[0][0].nbytes].tobytes() == host[0][0].tobytes()


# ---------------------------------------------------------------------------------------------- 8: a turntable
def test_four_turntable_eyes_on_one_scene(rtx, orc, samples_seeded, bunny):
    for v, frame, ost in vs.turntable(orc, samples_seeded):
        rgb, st = bunny["scene"].render_view(lib_view(rtx, v), stats=True)
        assert rgb.shape == (16, 24, 3) and np.array_equal(rgb, frame), v[1]
        assert st["primary_hits"] == ost["primary_hits"] and st["shadow_rays"] == ost["shadow_rays"], v[1]
