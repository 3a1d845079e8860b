"""GPU parity of relighting (rtx_render_view_lit, rtx_shade_rays_lit, their device-resident variants and the light kernel
behind them): a view or a ray batch of an uploaded scene under ANOTHER light and sample count against its expected values
(tests/light_sets.py, pinned to each other without a GPU by tests/test_light_sets.py) — render_pixel composed from oracle
pieces with that light, and, where one exists, the oracle scene created with it.  The tolerance is zero."""
import importlib
import os

import numpy as np
import pytest

import light_sets as ls
import query_sets as qs
import shade_sets as ss
import view_sets as vs
from query_sets import H, NO_HIT, W, bits

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUNNY = os.path.join(ROOT, "models", "big_bunny.obj")


@pytest.fixture(scope="module")
def rtx():
    mod = importlib.import_module("ray-tracer-rust_amd")
    assert mod.device_count() >= 1, "no HIP device: the product path has no CPU fallback"
    return mod


@pytest.fixture(scope="module")
def bunny(rtx, orc, samples_seeded):
    """big_bunny + ground created 32 x 32 with the default camera and light: the scene every bunny fixture is lit on"""
    scene = rtx.default_scene([BUNNY], W, H, samples_seeded)
    assert scene.info()["n_tris"] == 4969 and scene.light().nb_light_sample == 100
    yield scene
    scene.close()


def lib_view(rtx, v, rect=None):
    return rtx.Scene.view(v[0][0], v[0][1], rect=rect, **vs.camera(v))


def lib_light(rtx, fixture):
    return rtx.Scene.make_light(fixture["light"], fixture["count"])


def check_lit_view(scene, got, fx, what):
    """(rgb, shade, hits, stats) of a whole lit view against the composition, the oracle scene where the fixture has one, and
    rtx_trace_rays (the hits do not depend on the light)"""
    rgb, shade, hits, st = got
    s, w, h, nb = fx["set"], fx["w"], fx["h"], fx["nb_ray"]
    assert np.array_equal(rgb, fx["frame"]), "%s: bytes differ from the composition at (y, x) %s" % (
        what, np.argwhere((rgb != fx["frame"]).any(axis=2))[:8].tolist())
    if fx.get("oracle") is not None:
        assert np.array_equal(rgb, fx["oracle"][0]), what + ": bytes differ from the oracle scene created with that light"
    exp = s["shade"].reshape(h, w)
    bad = np.argwhere((bits(shade["linear"]) != bits(exp["linear"])).any(axis=2))
    assert not len(bad), "%s: linear differs at (y, x) %s" % (what, bad[:8].tolist())
    assert np.array_equal(shade["rgb8"], rgb) and np.array_equal(shade["hits"], exp["hits"]), what
    assert hits.tobytes() == scene.trace_rays(s["origins"], s["directions"], keep_order=True).tobytes(), what + ": out_hits is not rtx_trace_rays'"
    assert np.array_equal(hits["prim"].reshape(-1), s["hit"]["prim"]), what
    n_hits = int((s["hit"]["prim"] != NO_HIT).sum())
    assert st["primary_rays"] == w * h * nb and st["primary_hits"] == n_hits, (what, st)
    assert st["shadow_rays"] == fx["count"] * n_hits and st["rays"] == st["primary_rays"] + st["shadow_rays"], (what, st)
    if fx.get("oracle") is not None:
        assert st["primary_hits"] == fx["oracle"][1]["primary_hits"] and st["shadow_rays"] == fx["oracle"][1]["shadow_rays"], what


def render_lit(rtx, scene, fx):
    """the counted form with all three outputs, checked to give the uncounted form's bytes"""
    view, light = lib_view(rtx, fx["v"]), lib_light(rtx, fx)
    got = scene.render_view(view, stats=True, want_shade=True, want_hits=True, light=light)
    plain = scene.render_view(view, want_shade=True, want_hits=True, light=light)
    assert [x.tobytes() for x in plain] == [x.tobytes() for x in got[:3]], "with and without stats"
    assert np.array_equal(scene.render_view(view, light=light), got[0])                           # out_rgb alone
    return got


def all_fixture_lights(rtx, orc, samples):
    out = [(tri, count) for tri, count in ls.SIDE_LIGHTS.values()] + [(orc.LIGHT_TRI, c) for c in ls.OWN_COUNTS]
    out += [(ls.SIDE_LIGHTS["far_side"][0], ls.WRAP_COUNT), (ls.SOUP_LIGHT[0], 0)] + [(t, ls.ORBIT_COUNT) for t in ls.ORBIT_LIGHTS]
    return [rtx.Scene.make_light(tri, count) for tri, count in out]


# ---------------------------------------------------------------------------------------------- 1: the light kernel
def test_light_points_of_the_device_are_the_hosts(rtx, orc, samples_seeded, bunny):
    lights = all_fixture_lights(rtx, orc, samples_seeded)
    a = qs.scene_a(orc, samples_seeded)
    with rtx.default_scene([BUNNY], W, H, samples_seeded[:ls.WRAP_PAIRS], reference_tree=rtx.REFTREE_NEVER, tie_rank=None) as short, \
            rtx.Scene(*a["args"], nb_ray=2, **a["kw"]) as soup:
        for name, scene, nb_ray in (("bunny", bunny, 1), ("wrap", short, 1), ("soup", soup, 2)):
            for light in lights + [scene.light()]:
                want = scene.light_points_for(light)
                got = scene.debug_light_points(light)
                count = light.nb_light_sample or scene.light().nb_light_sample
                assert got.shape == want.shape == (nb_ray * count, 3), (name, count)
                assert np.array_equal(bits(got), bits(want)), (name, list(light.v0), count, np.argwhere(bits(got) != bits(want))[:4].tolist())
            assert np.array_equal(bits(scene.debug_light_points(scene.light())), bits(scene.light_points())), name
        # a large light after small ones (the buffer grows), and a small one again
        big = rtx.Scene.make_light(ls.SIDE_LIGHTS["grazing"][0], 70001)
        assert np.array_equal(bits(bunny.debug_light_points(big)), bits(bunny.light_points_for(big)))
        assert np.array_equal(bits(bunny.debug_light_points(lights[0])), bits(bunny.light_points_for(lights[0])))


# ---------------------------------------------------------------------------------------------- 2: lit views
@pytest.mark.parametrize("name", list(ls.SIDE_LIGHTS))
def test_side_under_another_light(rtx, orc, samples_seeded, bunny, name):
    fx = ls.side(orc, samples_seeded, name)
    check_lit_view(bunny, render_lit(rtx, bunny, fx), fx, name)


# ---------------------------------------------------------------------------------------------- 3: the scene's own light
def test_own_light_is_the_unlit_call(rtx, orc, samples_seeded, bunny):
    own = bunny.light()
    zero = bunny.light()
    zero.nb_light_sample = 0
    for v in (bunny.own_view(), lib_view(rtx, vs.BUNNY_VIEWS["side"]), lib_view(rtx, vs.BUNNY_VIEWS["side"], rect=(5, 3, 19, 13))):
        unlit = bunny.render_view(v, stats=True, want_shade=True, want_hits=True)
        for light in (own, zero):
            lit = bunny.render_view(v, stats=True, want_shade=True, want_hits=True, light=light)
            assert [x.tobytes() for x in lit[:3]] == [x.tobytes() for x in unlit[:3]]
            for k in ("primary_rays", "primary_hits", "shadow_rays", "rays", "box_tests", "tri_tests", "redo_tiles"):
                assert lit[3][k] == unlit[3][k], k
    assert np.array_equal(bunny.render_view(lib_view(rtx, vs.BUNNY_VIEWS["side"]), light=own),
                          vs.bunny_view(orc, samples_seeded, "side")["frame"])


# ---------------------------------------------------------------------------------------------- 4: counts, the wrapping table
@pytest.mark.parametrize("count", ls.OWN_COUNTS)
def test_own_triangle_with_another_count(rtx, orc, samples_seeded, bunny, count):
    fx = ls.side_count(orc, samples_seeded, count)
    check_lit_view(bunny, render_lit(rtx, bunny, fx), fx, "count %d" % count)


def test_sample_table_shorter_than_the_count(rtx, orc, samples_seeded):
    fx = ls.side_wrap(orc, samples_seeded)
    with rtx.default_scene([BUNNY], W, H, fx["samples"]) as scene:
        assert len(scene.samples) == ls.WRAP_PAIRS < fx["count"]
        check_lit_view(scene, render_lit(rtx, scene, fx), fx, "wrap")


# ---------------------------------------------------------------------------------------------- 5: the soup, two rays per pixel
def test_soup_with_spheres_and_two_rays_under_another_light(rtx, orc, samples_seeded):
    fx = ls.soup(orc, samples_seeded)
    a = fx["a"]
    with rtx.Scene(*a["args"], nb_ray=2, **a["kw"]) as scene:
        light = rtx.Scene.make_light(*ls.SOUP_LIGHT)                      # count 0: the scene's 24
        view = lib_view(rtx, fx["v"])
        got = scene.render_view(view, stats=True, want_shade=True, want_hits=True, light=light)
        assert got[2].shape == (22, 29, 2)
        check_lit_view(scene, got, fx, "soup")
        qs.check_normals(got[2].reshape(-1), fx["set"]["hit"], scene.normals(), a["kinds"], "lit soup view")
        explicit = scene.render_view(view, want_shade=True, light=rtx.Scene.make_light(ls.SOUP_LIGHT[0], 24))
        assert explicit[1].tobytes() == got[1].tobytes()


# ---------------------------------------------------------------------------------------------- 6: lit ray shading
@pytest.mark.parametrize("name", ["far_side", "distant"])
def test_shade_rays_under_another_light(rtx, orc, samples_seeded, bunny, name):
    fx = ls.side(orc, samples_seeded, name)
    s, light = fx["set"], lib_light(rtx, fx)
    n = len(s["shade"])
    assert n == 1188 and n % 64 != 0
    hits_by_trace = bunny.trace_rays(s["origins"], s["directions"], keep_order=True)
    for kw in (dict(keep_order=True), dict(force_regroup=True), dict()):
        shade, hits, st = bunny.shade_rays(s["origins"], s["directions"], want_hits=True, stats=True, light=light, **kw)
        assert shade.tobytes() == s["shade"].tobytes(), (name, kw, np.nonzero(shade != s["shade"])[0][:8])
        assert hits.tobytes() == hits_by_trace.tobytes(), (name, kw)
        n_hits = int((s["hit"]["prim"] != NO_HIT).sum())
        assert st["primary_rays"] == n and st["primary_hits"] == n_hits and st["shadow_rays"] == fx["count"] * n_hits, (kw, st)
        alone = bunny.shade_rays(s["origins"], s["directions"], light=light, **kw)                # out_hits NULL, no stats
        assert alone.tobytes() == s["shade"].tobytes(), (name, kw)
    # a batch that ends inside a wavefront, from the middle of the set
    part = ss.take(s, np.arange(200, 200 + 77))
    for kw in (dict(keep_order=True), dict(force_regroup=True)):
        assert bunny.shade_rays(part["origins"], part["directions"], light=light, **kw).tobytes() == part["shade"].tobytes(), kw


def test_shade_rays_on_the_soup_under_another_light(rtx, orc, samples_seeded):
    fx = ls.soup(orc, samples_seeded)
    a, s = fx["a"], fx["set"]
    with rtx.Scene(*a["args"], nb_ray=2, **a["kw"]) as scene:
        light = rtx.Scene.make_light(*ls.SOUP_LIGHT)
        for kw in (dict(keep_order=True), dict(force_regroup=True)):
            assert scene.shade_rays(s["origins"], s["directions"], light=light, **kw).tobytes() == s["shade"].tobytes(), kw


# ---------------------------------------------------------------------------------------------- 7: sequences
def test_a_sequence_of_lights_and_the_scene_afterwards(rtx, orc, samples_seeded):
    a, b = ls.side(orc, samples_seeded, "far_side"), ls.side(orc, samples_seeded, "point")
    a7 = dict(a, count=7)
    view = lib_view(rtx, a["v"])
    cam = ss.bunny_sets(orc, samples_seeded)["camera"]
    side = vs.bunny_view(orc, samples_seeded, "side")

    def usual(scene):
        shade, hits = scene.shade_rays(cam["origins"], cam["directions"], want_hits=True, force_regroup=True)
        return [scene.render_view(view, want_shade=True)[1].tobytes(), shade.tobytes(), hits.tobytes(), scene.render_rows().tobytes(),
                scene.render_view_rows(view).tobytes()]

    with rtx.default_scene([BUNNY], W, H, samples_seeded) as fresh:
        solo = usual(fresh)
    assert solo[1] == cam["shade"].tobytes() and solo[4] == side["frame"].tobytes()
    with rtx.default_scene([BUNNY], W, H, samples_seeded) as scene:
        frames = [scene.render_view(view, want_shade=True, light=lib_light(rtx, f))[1] for f in (a, b, a, a7)]
        for got, f in zip(frames[:3], (a, b, a)):
            assert got.reshape(-1).tobytes() == f["set"]["shade"].tobytes()
        assert frames[0].tobytes() == frames[2].tobytes() and frames[3].tobytes() != frames[0].tobytes()
        seven = scene.shade_rays(a["set"]["origins"], a["set"]["directions"], keep_order=True, light=lib_light(rtx, a7))
        assert frames[3].reshape(-1).tobytes() == seven.tobytes()          # A with another count: the view is the ray batch
        # two lights that differ in one vertex by the sign of a zero: each is its own
        plus, minus = list(ls.SIDE_LIGHTS["grazing"][0]), list(ls.SIDE_LIGHTS["grazing"][0])
        plus[6], minus[6] = 0.0, -0.0
        for tri in (plus, minus, plus):
            light = rtx.Scene.make_light(tri, 9)
            assert np.array_equal(bits(scene.debug_light_points(light)), bits(scene.light_points_for(light)))
            assert scene.render_view(view, want_shade=True, light=light)[1].reshape(-1).tobytes() == \
                scene.shade_rays(a["set"]["origins"], a["set"]["directions"], keep_order=True, light=light).tobytes()
        assert bytes(rtx.Scene.make_light(plus, 9)) != bytes(rtx.Scene.make_light(minus, 9))
        # afterwards the scene is what it was, through every path that reads the uploaded light
        assert usual(scene) == solo
        assert np.array_equal(bits(scene.light_points()), bits(scene.light_points_for(scene.light())))


# ---------------------------------------------------------------------------------------------- 8: device-resident
def test_device_resident_lit_calls_back_to_back_on_one_stream(rtx, orc, samples_seeded, bunny):
    torch = pytest.importorskip("torch")
    assert torch.cuda.is_available(), "torch sees no GPU"
    fxs = [ls.side(orc, samples_seeded, n) for n in ("far_side", "grazing")]
    view = lib_view(rtx, fxs[0]["v"])
    n = view.nx * view.ny
    stream = torch.cuda.Stream(device="cuda:0")
    assert stream.cuda_stream != torch.cuda.default_stream().cuda_stream
    with torch.cuda.stream(stream):
        bufs = [[torch.full((size + 16,), 0xAA, dtype=torch.uint8, device="cuda:0") for size in (n * 3, n * 16, n * 32)] for _ in fxs]
        stream.synchronize()
        with pytest.raises(rtx.RtxError) as e:
            bunny.render_view_device(0, view, bufs[0][0].data_ptr(), bufs[0][1].data_ptr() + 8, None, stream.cuda_stream, light=lib_light(rtx, fxs[0]))
        assert e.value.code == rtx.ERR_BAD_ARG
        # two lights, one library-owned light buffer, two sets of outputs, nothing waited for between
        for fx, b in zip(fxs, bufs):
            bunny.render_view_device(0, view, b[0].data_ptr(), b[1].data_ptr(), b[2].data_ptr(), stream.cuda_stream, light=lib_light(rtx, fx))
        # ... and a host lit call right behind them, on the library's stream: it waits for the event
        third = ls.side(orc, samples_seeded, "point")
        host = bunny.render_view(view, want_shade=True, light=lib_light(rtx, third))
        assert host[1].reshape(-1).tobytes() == third["set"]["shade"].tobytes()
        stream.synchronize()
        for fx, b in zip(fxs, bufs):
            rgb, shade, hits = (t.cpu().numpy() for t in b)
            assert rgb[:n * 3].tobytes() == fx["frame"].tobytes() and (rgb[n * 3:] == 0xAA).all()
            assert shade[:n * 16].tobytes() == fx["set"]["shade"].tobytes() and (shade[n * 16:] == 0xAA).all()
            assert np.array_equal(hits[:n * 32].view(rtx.rtx.RAY_HIT_DTYPE)["prim"], fx["set"]["hit"]["prim"]) and (hits[n * 32:] == 0xAA).all()
        # rtx_shade_rays_lit_device, regrouped, into a buffer of its own
        s = fxs[0]["set"]
        d_o, d_d = (torch.from_numpy(np.ascontiguousarray(x)).to("cuda:0") for x in (s["origins"], s["directions"]))
        d_shade = torch.full((n * 16 + 16,), 0xAA, dtype=torch.uint8, device="cuda:0")
        assert d_shade.data_ptr() % 16 == 0
        stream.synchronize()
        bunny.shade_rays_device(0, n, d_o.data_ptr(), d_d.data_ptr(), d_shade.data_ptr(), None, stream.cuda_stream,
                                force_regroup=True, light=lib_light(rtx, fxs[0]))
        stream.synchronize()
        out = d_shade.cpu().numpy()
        assert out[:n * 16].tobytes() == s["shade"].tobytes() and (out[n * 16:] == 0xAA).all()


# ---------------------------------------------------------------------------------------------- 9: an orbit of lights
def test_four_lights_on_an_orbit_of_one_scene(rtx, orc, samples_seeded, bunny):
    for k, fx in enumerate(ls.orbit(orc, samples_seeded)):
        got = bunny.render_view(lib_view(rtx, fx["v"]), stats=True, want_shade=True, want_hits=True, light=lib_light(rtx, fx))
        assert got[0].shape == (16, 24, 3)
        check_lit_view(bunny, got, fx, "orbit light %d" % k)
