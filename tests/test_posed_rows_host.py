"""The posed render pipeline without a GPU: the header, the exports and the bindings, where the plane kernel lives in
librtx.so, every argument check that needs no device — the twins' checks in the twins' order — the unchanged ISA of the
existing kernels, and the sanitizer leg of the host statements (the plane statement, the posed aimed stream)."""
import ctypes as C
import importlib
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import light_sets as ls
import lit_rows_sets as lr
import view_sets as vs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FUNCS = ("rtx_render_view_rows_posed", "rtx_render_view_rows_posed_device", "rtx_scene_posed_pipeline_records",
         "rtx_debug_pose_pipeline")
UNITS = ("rtx_kernel", "rtx_query", "rtx_shade", "rtx_view", "rtx_aim", "rtx_light", "rtx_tour", "rtx_pose")
F = np.float32


@pytest.fixture(scope="module")
def rtx():
    return importlib.import_module("ray-tracer-rust_amd")


@pytest.fixture(scope="module")
def scene(rtx, samples_half):
    """bunny + ground, 16 x 12 (test_view_rows_host's): the ground's 10,000 is the largest coordinate"""
    tris, rgb = rtx.default_primitives([os.path.join(ROOT, "models", "bunny.obj")])
    with rtx.Scene(16, 12, tris, rgb, samples_half[:64], tie_rank=None, eye=(3.0, 90.0, 210.0), look_at=(1.0, 20.0, -7.0),
                   up=(0.1, 1.0, 0.0), distance=40.0) as s:
        yield s


# ---------------------------------------------------------------------------------------------- header, exports, kernels
def test_header_declares_the_functions_and_the_library_exports_them(rtx):
    text = open(os.path.join(ROOT, "include", "rtx.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for f in FUNCS:
        assert re.search(r"\bint %s\s*\(" % f, hdr), f
    assert re.search(r"#define RTX_ABI_VERSION 3\b", hdr) and rtx.abi_version() == 3      # additions only
    assert "no posed form yet" not in text
    out = subprocess.check_output(["nm", "-D", "--defined-only", rtx.rtx.LIB_PATH], text=True)
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
    assert set(FUNCS) <= exported, set(FUNCS) - exported
    assert set(FUNCS) <= set(rtx.rtx._SIGS)
    rs = open(os.path.join(ROOT, "integration", "rtx_ffi.rs")).read()
    block = re.search(r'extern "C" \{(.*?)\n\}', rs, re.S).group(1)
    assert set(FUNCS) <= set(re.findall(r"pub fn (\w+)\(", block)), set(FUNCS) - set(re.findall(r"pub fn (\w+)\(", block))
    for m in ("posed_pipeline_records", "debug_pose_pipeline"):
        assert callable(getattr(rtx.Scene, m)), m
    for m in ("render_view_rows", "render_view_rows_device"):
        p = inspect.signature(getattr(rtx.Scene, m)).parameters
        assert "posed" in p and p["posed"].default is False, m
    assert C.sizeof(rtx.rtx.RtxView) == 76 and C.sizeof(rtx.rtx.RtxLight) == 40           # no new struct
    mk = open(os.path.join(ROOT, "ray-tracer-rust_amd", "csrc", "Makefile")).read()
    assert re.search(r"^UNITS\s*:=.*\brtx_planes\b", mk, re.M) and "rtx_planes.h" in mk   # the library and `make asm`


def test_the_plane_kernel_lives_in_its_own_namespace():
    """librtx.so carries exactly one rtxg:: kernel; the eight other namespaces' sets are what they were"""
    lib = os.path.join(ROOT, "ray-tracer-rust_amd", "librtx.so")
    blob = open(lib, "rb").read()

    def kernels(ns):
        return set(m.decode() for m in re.findall(rb"_ZN%d%s\d+([a-z0-9_]+_kernel(?:ILb[01]ELb[01]E)?)" % (len(ns), ns.encode()), blob)
                   if not m.startswith(b"__device_stub__"))

    forms = ["ILb%dELb%dE" % (c, s) for c in (0, 1) for s in (0, 1)]
    assert kernels("rtxg") == {"global_planes_kernel"}, kernels("rtxg")
    assert kernels("rtxp") == {"pose_records_kernel", "refit_short_kernel", "refit_long_kernel"}, kernels("rtxp")
    assert kernels("rtxt") == {"tour_kernel", "light_boxes_kernel"}, kernels("rtxt")
    assert kernels("rtxl") == {"light_points_kernel"}, kernels("rtxl")
    assert kernels("rtxa") == {"aim_order_kernel", "aim_place_kernel"}, kernels("rtxa")
    render = set(m.decode() for m in re.findall(rb"_ZN3rtx\d+([a-z0-9_]+_kernel)I?", blob) if not m.startswith(b"__device_stub__"))
    assert render == {"reset_kernel", "probe_kernel", "count_classes_kernel", "order_tiles_kernel", "shade_tiles_kernel",
                      "reference_tiles_kernel"}, render
    assert kernels("rtxq") == {"key_kernel"} | {k + f for k in ("closest_kernel", "occluded_kernel") for f in forms}, kernels("rtxq")
    assert kernels("rtxs") == {"shade_kernel" + f for f in forms}, kernels("rtxs")
    assert kernels("rtxv") == {"view_kernel" + f for f in forms}, kernels("rtxv")
    symbols = subprocess.run(["nm", "-C", lib], capture_output=True, text=True, check=True).stdout
    host_side = set(k for k in re.findall(r"\brtxg::(\w+_kernel)\(", symbols) if not k.startswith("__device_stub__"))
    assert host_side == {"global_planes_kernel"}, host_side


def test_existing_kernels_are_unchanged():
    """profiles/posed_rows_same_isa.txt: tools/same_isa.py over `make asm` of the parent commit and of this one, the eight
    existing units — one SAME line per kernel and no other verdict"""
    text = open(os.path.join(ROOT, "profiles", "posed_rows_same_isa.txt")).read()
    verdicts = re.findall(r"^(SAME|DIFF|MISSING)\b", text, re.M)
    assert len(verdicts) >= 23 and set(verdicts) == {"SAME"}, text
    for unit in UNITS:
        assert unit + ".gfx950.s" in text, unit
    assert set(re.findall(r"^exit status (\d+)", text, re.M)) == {"0"} and len(re.findall(r"^exit status", text, re.M)) == len(UNITS)
    for kernel in ("pose_records_kernel", "refit_short_kernel", "refit_long_kernel", "probe_kernel", "shade_tiles_kernel"):
        assert kernel in text, kernel
    assert "global_planes_kernel" not in text          # the new unit has no parent to compare with


# ---------------------------------------------------------------------------------------------- argument checks
def test_argument_checks_need_no_device(rtx, scene):
    """rtx_render_view_rows' checks for a NULL light, rtx_render_view_rows_lit's for a light, in their order: NULLs and the
    light's cap, the frame and full width, no rows, the eye's range and the light's vertices, d_bytes, then the device"""
    L = rtx.rtx._lib
    h = scene.handle
    BAD, OK, UNSUPPORTED, NO_DEVICE = rtx.ERR_BAD_ARG, rtx.OK, rtx.ERR_UNSUPPORTED, rtx.ERR_NO_DEVICE
    rgb = np.full(16 * 12 * 3, 7, np.uint8)
    own_light = scene.light()
    assert own_light.nb_light_sample == 100 and scene.nb_ray == 1

    def host(view, light=None, handle=h, out=rgb.ctypes.data, stats=None, device=99):
        return L.rtx_render_view_rows_posed(handle, device, C.byref(view) if view is not None else None,
                                            C.byref(light) if light is not None else None, out, stats)

    def device(view, light=None, handle=h, out=256, d_bytes=1 << 40, device=99):
        return L.rtx_render_view_rows_posed_device(handle, device, C.byref(view) if view is not None else None,
                                                   C.byref(light) if light is not None else None, out, d_bytes, None, None)

    def twin_host(view, light):
        if light is None:
            return L.rtx_render_view_rows(h, 99, C.byref(view), rgb.ctypes.data, None)
        return L.rtx_render_view_rows_lit(h, 99, C.byref(view), C.byref(light), rgb.ctypes.data, None)

    def twin_device(view, light, d_bytes=1 << 40):
        if light is None:
            return L.rtx_render_view_rows_device(h, 99, C.byref(view), 256, d_bytes, None, None)
        return L.rtx_render_view_rows_lit_device(h, 99, C.byref(view), C.byref(light), 256, d_bytes, None, None)

    def changed(**kw):
        v = scene.own_view()
        for k, x in kw.items():
            setattr(v, k, x)
        return v

    def light_with(count=100, **kw):
        out = rtx.Scene.make_light(ls.SIDE_LIGHTS["far_side"][0], count)
        for k, x in kw.items():
            setattr(out, k, (C.c_float * 3)(*x))
        return out

    own = scene.own_view()
    far = rtx.Scene.view(16, 12, **vs.camera(vs.BUNNY_VIEWS["far"]))
    nan_light = light_with(9, v0=(float("nan"), 0.0, 0.0))
    for call, twin in ((host, twin_host), (device, twin_device)):
        for light in (None, own_light):
            assert call(own, light, handle=None) == BAD and call(None, light) == BAD and call(own, light, out=None) == BAD
            assert call(own, light) == NO_DEVICE == twin(own, light)
            # a rectangle that is not the full width, rows outside the frame, frames without pixels
            for v in (changed(x0=1), changed(nx=15), changed(x0=1, nx=15), changed(nx=0), changed(nx=17), changed(y0=1), changed(ny=13),
                      changed(y0=0xFFFFFFF8, ny=12), changed(width=0, nx=0), changed(height=0, ny=0),
                      changed(width=1 << 16, nx=1 << 16, height=1 << 15)):
                assert call(v, light) == BAD == twin(v, light)
            # the eye's range rule, before a device is looked for
            for v in (far, changed(eye=(C.c_float * 3)(0.0, float("nan"), 0.0)), changed(eye=(C.c_float * 3)(0.0, 0.0, -10000.001))):
                assert call(v, light) == UNSUPPORTED == twin(v, light)
            assert call(changed(eye=(C.c_float * 3)(10000.0, -10000.0, 10000.0)), light) == NO_DEVICE
            # a frame that is wrong AND an eye out of range: the frame is looked at first
            assert call(changed(nx=15, eye=(C.c_float * 3)(3e4, 0.0, 0.0)), light) == BAD
        # the light's rules: the cap of 2^20 points ahead of everything else, the vertices with the eye
        assert call(own, light_with((1 << 20) + 1)) == BAD and call(own, light_with(0xFFFFFFFF)) == BAD
        assert call(None, light_with((1 << 20) + 1)) == BAD and call(changed(nx=15), light_with((1 << 20) + 1)) == BAD
        assert call(own, light_with(1 << 20)) == NO_DEVICE and call(own, light_with(0)) == NO_DEVICE
        for bad in (dict(v0=(float("nan"), 0.0, 0.0)), dict(v1=(0.0, float("inf"), 0.0)), dict(v2=(0.0, 0.0, float("-inf")))):
            assert call(own, light_with(9, **bad)) == UNSUPPORTED
        assert call(changed(nx=15), nan_light) == BAD and call(far, nan_light) == UNSUPPORTED
        distant = rtx.Scene.make_light(*ls.SIDE_LIGHTS["distant"])
        assert call(own, distant) == NO_DEVICE                      # no range rule on the light
        for tri in lr.OVERFLOW_LIGHTS:
            assert call(own, rtx.Scene.make_light(tri, 9)) == NO_DEVICE
    # the device variant's buffer: ny * width * 3 bytes at least, looked at before the rows' count and the eye
    for light in (None, own_light):
        assert device(own, light, d_bytes=16 * 12 * 3 - 1) == BAD and device(changed(y0=4, ny=5), light, d_bytes=16 * 5 * 3 - 1) == BAD
        assert device(changed(y0=4, ny=5), light, d_bytes=16 * 5 * 3) == NO_DEVICE
        assert device(far, light, d_bytes=5) == BAD == twin_device(far, light, d_bytes=5)
    # no rows: fine, nothing written, stats zeroed — with no device at all, whatever the eye and the vertices
    st = rtx.rtx.Stats()
    for v in (changed(ny=0), changed(y0=12, ny=0), changed(ny=0, eye=(C.c_float * 3)(3e4, 0.0, 0.0))):
        for light in (None, own_light, light_with(7), nan_light):
            st.primary_rays, st.kernel_ms, st.shadow_rays = 5, 3.0, 9
            assert host(v, light) == OK and device(v, light) == OK and device(v, light, d_bytes=0) == OK
            assert host(v, light, stats=C.byref(st)) == OK
            assert st.primary_rays == 0 and st.rays == 0 and st.primary_hits == 0 and st.shadow_rays == 0 and st.kernel_ms == 0.0
        assert host(v, light_with((1 << 20) + 1)) == BAD
    assert (rgb == 7).all()
    assert scene.render_view_rows(changed(ny=0), posed=True).shape == (0, 16, 3)
    assert scene.render_view_rows(changed(ny=0), posed=True, light=own_light).shape == (0, 16, 3)
    if rtx.device_count() == 0:
        assert host(own, device=0) == NO_DEVICE and device(own, device=0) == NO_DEVICE
        with pytest.raises(rtx.RtxError) as e:
            scene.render_view_rows(own, stats=True, posed=True)
        assert e.value.code == NO_DEVICE
    with pytest.raises(rtx.RtxError) as e:
        scene.render_view_rows(far, posed=True)
    assert e.value.code == UNSUPPORTED

    # rtx_scene_posed_pipeline_records and rtx_debug_pose_pipeline
    f32p, u32p = rtx.rtx.f32p, rtx.rtx.u32p
    pose = np.ascontiguousarray(scene.tris.copy())
    vp = pose.ctypes.data_as(f32p)
    eye = np.array([1.0, 2.0, 3.0], F)
    ep = eye.ctypes.data_as(f32p)
    info = scene.info()
    planes, aimed = np.zeros((info["n_global"], 16), np.uint32), np.zeros((info["n_nodes"], 8), np.uint32)
    pp, ap = planes.ctypes.data_as(u32p), aimed.ctypes.data_as(u32p)
    assert L.rtx_scene_posed_pipeline_records(None, vp, ep, pp, ap) == BAD
    assert L.rtx_scene_posed_pipeline_records(h, None, ep, pp, ap) == BAD
    assert L.rtx_scene_posed_pipeline_records(h, vp, None, pp, ap) == BAD                  # an aimed stream needs an eye
    assert not planes.any() and not aimed.any()
    assert L.rtx_scene_posed_pipeline_records(h, vp, None, None, None) == OK               # each output may be NULL
    assert L.rtx_scene_posed_pipeline_records(h, vp, None, pp, None) == OK and planes.any() and not aimed.any()
    assert L.rtx_scene_posed_pipeline_records(h, vp, ep, None, ap) == OK and aimed.any()
    assert np.array_equal(aimed, scene.aimed_nodes(eye))                                   # the identity pose
    assert L.rtx_debug_pose_pipeline(None, 99, ep, pp, ap) == BAD and L.rtx_debug_pose_pipeline(h, 99, None, pp, ap) == BAD
    assert L.rtx_debug_pose_pipeline(h, 99, ep, pp, ap) == NO_DEVICE and L.rtx_debug_pose_pipeline(h, 99, None, pp, None) == NO_DEVICE
    with pytest.raises(ValueError):
        scene.posed_pipeline_records(pose[:-1])


# ---------------------------------------------------------------------------------------------- sanitizers
def test_host_statements_are_clean_under_asan_and_ubsan(tmp_path):
    out = subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "tests", "sanitize_posed_rows"), "run", "OUT=%s" % tmp_path],
                         capture_output=True, text=True, timeout=900)
    text = out.stdout + out.stderr
    assert out.returncode == 0, text[-4000:]
    assert "posed rows sanitizer driver: 0 failed checks" in text
    assert "ERROR: AddressSanitizer" not in text and "runtime error" not in text and "LeakSanitizer" not in text, text[-4000:]
