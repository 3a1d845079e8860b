"""Relighting without a GPU: the header, the exports and the bindings of the seven entry points, RtxLight's layout, where
the light kernel lives in librtx.so, every argument check that needs no device, the host statement of the light kernel
(rtx_scene_light_points_for) against rtx_scene_light_points of scenes CREATED with the light and against the oracle's
get_sample, and the conditions the fixtures of tests/light_sets.py must meet to test what they are for — the composition
pinned to the three oracle scenes among them.  Nothing here takes a tolerance."""
import ctypes as C
import importlib
import os
import re
import subprocess

import numpy as np
import pytest

import light_sets as ls
import view_sets as vs
from query_sets import bits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FUNCS = ("rtx_scene_light", "rtx_scene_light_points_for", "rtx_debug_light_points", "rtx_render_view_lit",
         "rtx_render_view_lit_device", "rtx_shade_rays_lit", "rtx_shade_rays_lit_device")
FIELDS = [("v0", 0, 12), ("v1", 12, 12), ("v2", 24, 12), ("nb_light_sample", 36, 4)]       # name, offset, size
RENDER_KERNELS = {"reset_kernel", "probe_kernel", "count_classes_kernel", "order_tiles_kernel", "shade_tiles_kernel",
                  "reference_tiles_kernel"}
CREATED = dict(eye=(3.0, 90.0, 210.0), look_at=(1.0, 20.0, -7.0), up=(0.1, 1.0, 0.0), distance=40.0)


@pytest.fixture(scope="module")
def rtx():
    return importlib.import_module("ray-tracer-rust_amd")


@pytest.fixture(scope="module")
def prims(rtx):
    return rtx.default_primitives([os.path.join(ROOT, "models", "bunny.obj")])


def small_scene(rtx, prims, samples, **kw):
    """bunny + ground, 16 x 12, no reference tree: cheap to create with any light, count, nb_ray and table"""
    return rtx.Scene(16, 12, prims[0], prims[1], samples, tie_rank=None, **dict(CREATED, **kw))


@pytest.fixture(scope="module")
def scene(rtx, prims, samples_seeded):
    with small_scene(rtx, prims, samples_seeded[:4096]) as s:
        yield s


# ---------------------------------------------------------------------------------------------- header, exports, layout
def test_header_declares_the_functions_and_the_library_exports_them(rtx):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rtx.h")).read(), flags=re.S)
    for f in FUNCS:
        assert re.search(r"\bint %s\s*\(" % f, hdr), f
    assert re.search(r"#define RTX_ABI_VERSION 3\b", hdr) and rtx.abi_version() == 3      # additions only
    out = subprocess.check_output(["nm", "-D", "--defined-only", rtx.rtx.LIB_PATH], text=True)
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
    assert set(FUNCS) <= exported, set(FUNCS) - exported
    assert set(FUNCS) <= set(rtx.rtx._SIGS)
    rs = open(os.path.join(ROOT, "integration", "rtx_ffi.rs")).read()
    block = re.search(r'extern "C" \{(.*?)\n\}', rs, re.S).group(1)
    assert set(FUNCS) <= set(re.findall(r"pub fn (\w+)\(", block))


def test_light_layout_in_c_ctypes_and_rust(rtx, tmp_path):
    src = tmp_path / "light.c"
    names = [n for n, _, _ in FIELDS]
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "rtx.h"\nint main(void) {\n'
                   'printf("%zu %zu\\n", sizeof(RtxLight), _Alignof(RtxLight));\n' +
                   "".join('printf("%s %%zu %%zu\\n", offsetof(RtxLight, %s), sizeof(((RtxLight *)0)->%s));\n' % (n, n, n) for n in names) +
                   'return 0; }\n')
    exe = tmp_path / "light"
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    lines = subprocess.check_output([str(exe)], text=True).splitlines()
    assert lines[0].split() == ["40", "4"]
    assert [(l.split()[0], int(l.split()[1]), int(l.split()[2])) for l in lines[1:]] == FIELDS
    T = rtx.rtx.RtxLight
    assert C.sizeof(T) == 40 and C.alignment(T) == 4
    assert [(n, getattr(T, n).offset, getattr(T, n).size) for n, _ in T._fields_] == FIELDS
    rs = open(os.path.join(ROOT, "integration", "rtx_ffi.rs")).read()
    m = re.search(r"#\[repr\(C\)\]\s*(?:#\[derive\([^\)]*\)\]\s*)?pub struct RtxLight \{(.*?)\n\}", rs, re.S)
    assert m, "RtxLight with #[repr(C)] not found in rtx_ffi.rs"
    rust = {"u32": 4, "[f32; 3]": 12}
    got, offset = [], 0
    for n, t in re.findall(r"pub (\w+): ([^,\n]+),", m.group(1)):         # every member is 4-byte aligned: no padding
        got.append((n, offset, rust[t]))
        offset += rust[t]
    assert got == FIELDS and offset == 40


def test_light_kernel_lives_in_its_own_namespace():
    """librtx.so carries exactly one rtxl:: kernel; the other namespaces' sets are what they were"""
    lib = os.path.join(ROOT, "ray-tracer-rust_amd", "librtx.so")
    blob = open(lib, "rb").read()

    def kernels(ns):
        return set(m.decode() for m in re.findall(rb"_ZN%d%s\d+([a-z0-9_]+_kernel(?:ILb[01]ELb[01]E)?)" % (len(ns), ns.encode()), blob)
                   if not m.startswith(b"__device_stub__"))

    forms = ["ILb%dELb%dE" % (c, s) for c in (0, 1) for s in (0, 1)]
    assert kernels("rtxl") == {"light_points_kernel"}, kernels("rtxl")
    render = set(m.decode() for m in re.findall(rb"_ZN3rtx\d+([a-z0-9_]+_kernel)I?", blob) if not m.startswith(b"__device_stub__"))
    assert render == RENDER_KERNELS, render
    assert kernels("rtxq") == {"key_kernel"} | {k + f for k in ("closest_kernel", "occluded_kernel") for f in forms}, kernels("rtxq")
    assert kernels("rtxs") == {"shade_kernel" + f for f in forms}, kernels("rtxs")
    assert kernels("rtxv") == {"view_kernel" + f for f in forms}, kernels("rtxv")
    assert kernels("rtxa") == {"aim_order_kernel", "aim_place_kernel"}, kernels("rtxa")
    symbols = subprocess.run(["nm", "-C", lib], capture_output=True, text=True, check=True).stdout
    host_side = set(k for k in re.findall(r"\brtxl::(\w+_kernel)\(", symbols) if not k.startswith("__device_stub__"))
    assert host_side == {"light_points_kernel"}, host_side
    undefined = subprocess.run(["nm", "-D", "--undefined-only", lib], capture_output=True, text=True, check=True).stdout
    assert "getenv" not in undefined


# ---------------------------------------------------------------------------------------------- argument checks
def test_argument_checks_need_no_device(rtx, scene):
    L, R = rtx.rtx._lib, rtx.rtx
    h = scene.handle
    BAD, OK, UNSUPPORTED, NO_DEVICE = rtx.ERR_BAD_ARG, rtx.OK, rtx.ERR_UNSUPPORTED, rtx.ERR_NO_DEVICE
    own_view, own = scene.own_view(), scene.light()
    rgb = np.full(16 * 12 * 3, 7, np.uint8)
    n = 5
    o, d = np.zeros((n, 3), np.float32), np.ones((n, 3), np.float32)
    shade = np.full(n * 16, 7, np.uint8)
    f32p = C.POINTER(C.c_float)

    def ref(x):
        return C.byref(x) if x is not None else None

    # device 99 is none on any machine: a call that gets as far as looking for its device answers NO_DEVICE
    def view(light, v=own_view, handle=h, out=rgb.ctypes.data, stats=None):
        return L.rtx_render_view_lit(handle, 99, ref(v), ref(light), out, None, None, stats)

    def view_dev(light, v=own_view, handle=h, out=256):
        return L.rtx_render_view_lit_device(handle, 99, ref(v), ref(light), out, None, None, None)

    def rays(light, handle=h, n_pixels=n, flags=0, out=shade.ctypes.data_as(C.POINTER(R.PixelShade)), stats=None):
        return L.rtx_shade_rays_lit(handle, 99, n_pixels, o.ctypes.data_as(f32p), d.ctypes.data_as(f32p), flags, ref(light), out, None, stats)

    def rays_dev(light, handle=h, n_pixels=n, flags=0, out=256):
        return L.rtx_shade_rays_lit_device(handle, 99, n_pixels, 512, 1024, flags, ref(light), out, None, None)

    calls = (view, view_dev, rays, rays_dev)
    for call in calls:
        assert call(own) == NO_DEVICE                                        # the scene's own light passes every check
        assert call(None) == BAD and call(own, handle=None) == BAD and call(own, out=None) == BAD
    # the twins' own checks come with them
    assert view(own, v=None) == BAD and view_dev(own, v=None) == BAD
    wide = scene.own_view()
    wide.nx = 17
    assert view(own, v=wide) == BAD and view_dev(own, v=wide) == BAD
    assert rays(own, flags=4) == BAD and rays_dev(own, flags=4) == BAD
    assert view_dev(own, out=256) == NO_DEVICE
    assert L.rtx_render_view_lit_device(h, 99, C.byref(own_view), C.byref(own), 256, 264, None, None) == BAD      # d_shade 16-byte aligned
    assert L.rtx_shade_rays_lit_device(h, 99, n, 514, 1024, 0, C.byref(own), 256, None, None) == BAD              # floats 4-byte aligned
    # at most 2^20 light points: nb_ray = 1 here
    assert ls.MAX_POINTS == 1 << 20
    at_cap, over = R.Scene.make_light(rtx.DEFAULT_LIGHT, 1 << 20), R.Scene.make_light(rtx.DEFAULT_LIGHT, (1 << 20) + 1)
    for call in calls:
        assert call(at_cap) == NO_DEVICE and call(over) == BAD and call(R.Scene.make_light(rtx.DEFAULT_LIGHT, 0xFFFFFFFF)) == BAD
    # a vertex that is not finite: UNSUPPORTED, decided before a device is looked for
    for k in range(9):
        for bad in (float("nan"), float("inf"), -float("inf")):
            tri = list(rtx.DEFAULT_LIGHT)
            tri[k] = bad
            light = R.Scene.make_light(tri, 3)
            for call in calls:
                assert call(light) == UNSUPPORTED, (k, bad)
            assert L.rtx_debug_light_points(h, 99, C.byref(light), o.ctypes.data_as(f32p)) == UNSUPPORTED
    # ... but the argument checks come first
    nan = R.Scene.make_light((float("nan"),) * 9, 3)
    assert view(nan, v=wide) == BAD and rays(nan, flags=4) == BAD
    nan_over = R.Scene.make_light((float("nan"),) * 9, (1 << 20) + 1)
    assert view(nan_over) == BAD and rays_dev(nan_over) == BAD
    # no pixels: fine, nothing written, stats zeroed — with no device at all, whatever the light's vertices
    st = R.Stats()
    for light in (own, nan, R.Scene.make_light(ls.SIDE_LIGHTS["distant"][0], 7)):
        for v in ((0, 12), (16, 0), (0, 0)):
            empty = scene.own_view()
            empty.nx, empty.ny = v
            st.primary_rays, st.shadow_rays, st.kernel_ms = 5, 9, 3.0
            assert view(light, v=empty) == OK and view_dev(light, v=empty) == OK
            assert view(light, v=empty, stats=C.byref(st)) == OK
            assert st.primary_rays == 0 and st.rays == 0 and st.primary_hits == 0 and st.shadow_rays == 0 and st.kernel_ms == 0.0
        st.primary_rays, st.shadow_rays, st.kernel_ms = 5, 9, 3.0
        assert rays(light, n_pixels=0) == OK and rays_dev(light, n_pixels=0) == OK
        assert rays(light, n_pixels=0, stats=C.byref(st)) == OK
        assert st.primary_rays == 0 and st.rays == 0 and st.primary_hits == 0 and st.shadow_rays == 0 and st.kernel_ms == 0.0
    assert (rgb == 7).all() and (shade == 7).all()
    # a light beyond the scene's largest coordinate is no error: there is no range rule on the light
    far = R.Scene.make_light(ls.SIDE_LIGHTS["distant"][0], 7)
    assert max(abs(x) for x in ls.SIDE_LIGHTS["distant"][0]) == 30000.0 > vs.SCENE_BOUND
    for call in calls:
        assert call(far) == NO_DEVICE
    # the read-back, the host statement and the diagnostic
    assert L.rtx_scene_light(None, C.byref(own)) == BAD and L.rtx_scene_light(h, None) == BAD
    assert L.rtx_scene_light_points_for(None, C.byref(own), None) == BAD and L.rtx_scene_light_points_for(h, None, None) == BAD
    assert L.rtx_scene_light_points_for(h, C.byref(over), None) == BAD
    assert L.rtx_scene_light_points_for(h, C.byref(at_cap), None) == 1 << 20
    assert L.rtx_scene_light_points_for(h, C.byref(own), None) == 100 == scene.info()["n_light_points"]
    out = o.ctypes.data_as(f32p)
    assert L.rtx_debug_light_points(None, 99, C.byref(own), out) == BAD and L.rtx_debug_light_points(h, 99, None, out) == BAD
    assert L.rtx_debug_light_points(h, 99, C.byref(own), None) == BAD and L.rtx_debug_light_points(h, 99, C.byref(over), out) == BAD
    assert L.rtx_debug_light_points(h, 99, C.byref(own), out) == NO_DEVICE
    if rtx.device_count() == 0:
        with pytest.raises(rtx.RtxError) as e:
            scene.render_view(own_view, light=own)
        assert e.value.code == NO_DEVICE
    with pytest.raises(rtx.RtxError) as e:
        scene.shade_rays(o, d, light=nan)
    assert e.value.code == UNSUPPORTED


# ---------------------------------------------------------------------------------------------- the host statement
def test_scene_light_is_what_the_scene_was_created_with(rtx, prims, samples_seeded, scene):
    own = scene.light()
    assert list(own.v0) + list(own.v1) + list(own.v2) == list(rtx.DEFAULT_LIGHT) and own.nb_light_sample == 100
    assert bytes(rtx.Scene.make_light(rtx.DEFAULT_LIGHT, 100)) == bytes(own)
    tri = (1.5, -2.25, 3.0, -0.0, 1e-30, 7.0, 1e30, 8.0, -9.5)
    with small_scene(rtx, prims, samples_seeded[:64], light_tri=tri, nb_light_sample=3) as s:
        got = s.light()
        assert bytes(got) == bytes(rtx.Scene.make_light(tri, 3))             # bit for bit, the -0.0 included
        assert np.signbit(got.v1[0])


def test_points_of_the_own_light_are_the_scenes(rtx, prims, samples_seeded, scene):
    for s in (scene,):
        assert np.array_equal(bits(s.light_points_for(s.light())), bits(s.light_points()))
        zero = s.light()
        zero.nb_light_sample = 0                                             # 0 = the scene's
        assert np.array_equal(bits(s.light_points_for(zero)), bits(s.light_points()))
    with small_scene(rtx, prims, samples_seeded[:7], nb_ray=3, nb_light_sample=19, light_tri=ls.SIDE_LIGHTS["grazing"][0]) as s:
        assert s.light_points().shape == (57, 3)
        assert np.array_equal(bits(s.light_points_for(s.light())), bits(s.light_points()))


@pytest.mark.parametrize("nb_ray, pairs", [(1, 4096), (2, 4096), (1, ls.WRAP_PAIRS), (3, 2)])
def test_points_of_another_light_are_those_of_a_scene_created_with_it(rtx, orc, prims, samples_seeded, nb_ray, pairs):
    """rtx_scene_light_points_for(L, n) on a scene created with the default light == rtx_scene_light_points of a scene
    created with L and n (the same table, the same nb_ray), and == the oracle's get_sample of table entry (r*nb_ray + i) % len"""
    table = np.ascontiguousarray(samples_seeded[:pairs])
    lights = list(ls.SIDE_LIGHTS.values()) + [(orc.LIGHT_TRI, c) for c in ls.OWN_COUNTS] + \
        [(ls.SIDE_LIGHTS["far_side"][0], ls.WRAP_COUNT), (ls.SOUP_LIGHT[0], 24)] + [(t, ls.ORBIT_COUNT) for t in ls.ORBIT_LIGHTS]
    with small_scene(rtx, prims, table, nb_ray=nb_ray) as base:
        for tri, count in lights:
            got = base.light_points_for(rtx.Scene.make_light(tri, count))
            assert got.shape == (nb_ray * count, 3)
            with small_scene(rtx, prims, table, nb_ray=nb_ray, light_tri=tri, nb_light_sample=count) as made:
                assert np.array_equal(bits(got), bits(made.light_points())), (tri, count)
            assert np.array_equal(bits(got), bits(ls.points(orc, tri, table, nb_ray, count))), (tri, count)
        if pairs < ls.WRAP_COUNT:                                            # the index wraps: point i + pairs is point i
            got = base.light_points_for(rtx.Scene.make_light(ls.SIDE_LIGHTS["far_side"][0], ls.WRAP_COUNT))
            assert nb_ray * nb_ray + ls.WRAP_COUNT > pairs
            assert np.array_equal(bits(got[:ls.WRAP_COUNT - pairs]), bits(got[pairs:ls.WRAP_COUNT]))
        if nb_ray == 2:                                                      # ray 1 starts at table entry r * nb_ray = 2
            got = base.light_points_for(rtx.Scene.make_light(ls.SOUP_LIGHT[0], 24)).reshape(2, 24, 3)
            assert np.array_equal(bits(got[1, :22]), bits(got[0, 2:])) and not np.array_equal(bits(got[1]), bits(got[0]))


def test_a_point_light_is_not_a_point():
    """get_sample's weights are 1 - sqrt(u), sqrt(u) (1 - sqrt(v)) and v sqrt(u): they do not sum to one (the reference has
    it so), and v0 == v1 == v2 gives samples along the line through the origin and the vertex — fixture (d) is no shortcut"""
    tri, count = ls.SIDE_LIGHTS["point"]
    assert tri[0:3] == tri[3:6] == tri[6:9]


# ---------------------------------------------------------------------------------------------- fixture conditions
def test_side_fixtures_hold_what_they_are_for(orc, samples_seeded):
    own = vs.bunny_view(orc, samples_seeded, "side")
    hits = own["set"]["shade"]["hits"]
    for name in ls.SIDE_LIGHTS:
        r = ls.side(orc, samples_seeded, name)
        s = r["set"]
        assert r["frame"].shape == (27, 44, 3) and np.array_equal(s["shade"]["hits"], hits)       # the hits do not depend on the light
        assert s["hit"].tobytes() == own["set"]["hit"].tobytes()
        assert (r["frame"] != own["frame"]).any(), name + ": a lit call that ignored its light would pass"
        assert np.array_equal(s["samples"], hits.astype(np.int64) * r["count"])
        if name in ls.PARTLY_LIT:
            assert ls.partly_lit(s) > 0, name
    a = ls.side(orc, samples_seeded, "far_side")
    assert np.array_equal(a["frame"], a["oracle"][0]), "composition and oracle scene disagree under the moved light"
    assert a["oracle"][1]["primary_hits"] == int(hits.sum()) and a["oracle"][1]["shadow_rays"] == 100 * int(hits.sum())
    # (a) moves the ground shadow: ground pixels in the shadow of one light are lit by the other
    ground = (own["set"]["hit"]["prim"] == 4968)
    dark_own, dark_moved = ground & (own["set"]["lit"] == 0), ground & (a["set"]["lit"] == 0)
    assert dark_own.any() and dark_moved.any() and (dark_own & (a["set"]["lit"] == 100)).any() and (dark_moved & (own["set"]["lit"] == 100)).any()
    # (c) lies beyond the scene's bound
    assert max(abs(x) for x in ls.SIDE_LIGHTS["distant"][0]) > vs.SCENE_BOUND


def test_counts_and_the_wrapping_table(orc, samples_seeded):
    own = vs.bunny_view(orc, samples_seeded, "side")
    hits = int(own["set"]["shade"]["hits"].sum())
    frames = {}
    for count in ls.OWN_COUNTS:
        r = ls.side_count(orc, samples_seeded, count)
        assert int(r["set"]["samples"].sum()) == count * hits
        frames[count] = r["frame"]
        assert (r["frame"] != own["frame"]).any(), count
    assert (frames[7] != own["frame"]).any(axis=2).sum() >= 1                # count 7 against the scene's 100
    assert set(ls.OWN_COUNTS) == {1, 7, 130} and 130 > orc.NB_LIGHT_SAMPLE
    w = ls.side_wrap(orc, samples_seeded)
    assert len(w["samples"]) == ls.WRAP_PAIRS < ls.WRAP_COUNT
    assert (w["frame"] != own["frame"]).any() and ls.partly_lit(w["set"]) > 0
    # the short table changes the rays too: the fixture's own hits, not the seeded table's
    assert not np.array_equal(w["set"]["directions"], own["set"]["directions"])


def test_soup_and_orbit_fixtures(orc, samples_seeded):
    so, own = ls.soup(orc, samples_seeded), vs.soup_view(orc, samples_seeded)
    assert so["nb_ray"] == 2 and so["count"] == 24 and ls.SOUP_LIGHT[1] == 0
    assert so["set"]["hit"].tobytes() == own["set"]["hit"].tobytes() and (so["frame"] != own["frame"]).any()
    assert vs.sphere_rays(own) > 0 and ls.partly_lit(so["set"]) > 0
    assert (so["set"]["shade"]["hits"] == 2).any()                           # pixels whose ray 1 reads light points [1][*]
    lights = ls.orbit(orc, samples_seeded)
    own_frame = vs.turntable(orc, samples_seeded)[0][1]                      # ORBIT_VIEW under the scene's own light
    assert len(lights) == 4 and ls.ORBIT_VIEW[1] == vs.TURNTABLE_EYES[0]
    for k, r in enumerate(lights):
        assert r["frame"].shape == (16, 24, 3) and (r["frame"] != own_frame).any(), k
        assert (r["oracle"] is not None) == (k in ls.ORBIT_ORACLE)
        if r["oracle"] is not None:
            assert np.array_equal(r["frame"], r["oracle"][0]), "orbit light %d: composition and oracle scene disagree" % k
            assert r["oracle"][1]["shadow_rays"] == ls.ORBIT_COUNT * r["oracle"][1]["primary_hits"]
    for j in range(4):
        for k in range(j):
            assert (lights[j]["frame"] != lights[k]["frame"]).any(), (j, k)
