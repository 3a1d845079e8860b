"""The render pipeline's record output without a GPU: the header, the exports and the bindings, where the record forms of
the kernels live in librtx.so, every argument check that needs no device — the byte twins' checks in the twins' order, and
the call's own — and the unchanged ISA of the existing kernels."""
import ctypes as C
import importlib
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import light_sets as ls
import view_sets as vs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FUNCS = ("rtx_render_view_rows_shade", "rtx_render_view_rows_shade_device")
UNITS = ("rtx_kernel", "rtx_query", "rtx_shade", "rtx_view", "rtx_aim", "rtx_light", "rtx_tour", "rtx_pose", "rtx_planes",
         "rtx_rebuild", "rtx_prims", "rtx_move", "rtx_skin", "rtx_samples", "rtx_accum")
RECORD_KERNELS = {"probe_records_kernel", "shade_records_kernel", "reference_records_kernel"}


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
    hdr = " ".join(re.sub(r"/\*.*?\*/", "", text, flags=re.S).split())
    assert ("int rtx_render_view_rows_shade(RtxScene *scene, int device, const RtxView *view, const RtxLight *light , "
            "uint32_t flags , RtxPixelShade *out_shade, RtxStats *stats);") in hdr
    assert ("int rtx_render_view_rows_shade_device(RtxScene *scene, int device, const RtxView *view, const RtxLight *light, "
            "uint32_t flags, void *d_shade, size_t d_bytes, void *stream, uint64_t *d_counters);") in hdr
    assert re.search(r"#define RTX_ROWS_POSED 1u\b", hdr) and rtx.rtx.ROWS_POSED == 1
    assert re.search(r"#define RTX_ABI_VERSION 3\b", hdr) and rtx.abi_version() == 3      # additions only
    out = subprocess.check_output(["nm", "-D", "--defined-only", rtx.rtx.LIB_PATH], text=True)
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
    assert set(FUNCS) <= exported, set(FUNCS) - exported
    assert set(FUNCS) <= set(rtx.rtx._SIGS)
    rs = open(os.path.join(ROOT, "integration", "rtx_ffi.rs")).read()
    block = re.search(r'extern "C" \{(.*?)\n\}', rs, re.S).group(1)
    assert set(FUNCS) <= set(re.findall(r"pub fn (\w+)\(", block))
    assert re.search(r"pub const RTX_ROWS_POSED: u32 = 1;", rs)
    for m in ("render_view_rows_shade", "render_view_rows_shade_device"):
        p = inspect.signature(getattr(rtx.Scene, m)).parameters
        assert p["posed"].default is False and p["light"].default is None, m
    assert C.sizeof(rtx.rtx.PixelShade) == 16 and rtx.PIXEL_SHADE_DTYPE.itemsize == 16          # no new struct
    for doc in ("INTEGRATION.md", "README.md", "DESIGN.md"):
        assert "rtx_render_view_rows_shade" in open(os.path.join(ROOT, doc)).read(), doc


def test_the_record_forms_live_in_their_own_namespace():
    """librtx.so carries the three rtxo:: kernels — probe_kernel's one-wavefront form only: a view's launch has no long list —
    and the render pipeline's own namespace holds the six kernels it held"""
    lib = os.path.join(ROOT, "ray-tracer-rust_amd", "librtx.so")
    blob = open(lib, "rb").read()
    records = set(m.decode() for m in re.findall(rb"_ZN4rtxo\d+([a-z0-9_]+_kernel)I", blob) if not m.startswith(b"__device_stub__"))
    assert records == RECORD_KERNELS, records
    render = set(m.decode() for m in re.findall(rb"_ZN3rtx\d+([a-z0-9_]+_kernel)I?", blob) if not m.startswith(b"__device_stub__"))
    assert render == {"reset_kernel", "probe_kernel", "count_classes_kernel", "order_tiles_kernel", "shade_tiles_kernel",
                      "reference_tiles_kernel"}, render
    # COUNT x SPHERES x WHOLE of the two kernels that have a whole-stream form, COUNT x SPHERES of the third, FAST always
    forms = set(m.decode() for m in re.findall(rb"_ZN4rtxo\d+((?:probe|shade)_records_kernelI[A-Za-z0-9]+?)EEv", blob))
    assert forms == {"probe_records_kernelILb%dELb1ELb%dELb%dE" % (c, s, w) for c in (0, 1) for s in (0, 1) for w in (0, 1)} | \
        {"shade_records_kernelILb%dELb1ELi8ELb%dELb%dE" % (c, s, w) for c in (0, 1) for s in (0, 1) for w in (0, 1)}, forms
    for ns, want in (("rtxa", {"aim_order_kernel", "aim_place_kernel"}), ("rtxl", {"light_points_kernel"}),
                     ("rtxt", {"tour_kernel", "light_boxes_kernel"}), ("rtxg", {"global_planes_kernel"})):
        got = set(m.decode() for m in re.findall(rb"_ZN%d%s\d+([a-z0-9_]+_kernel)" % (len(ns), ns.encode()), blob)
                  if not m.startswith(b"__device_stub__"))
        assert got == want, (ns, got)


def test_existing_kernels_are_unchanged():
    """profiles/rows_shade_same_isa.txt: tools/same_isa.py over `make asm` of the parent commit and of this one — every
    symbol the parent has is SAME, and the symbols only this commit has are the record forms, named as the new ones"""
    text = open(os.path.join(ROOT, "profiles", "rows_shade_same_isa.txt")).read()
    lines = [l.strip() for l in text.splitlines() if re.match(r"\s*(SAME|DIFF|MISSING)\b", l)]
    assert len([l for l in lines if l.startswith("SAME")]) >= 460 and not [l for l in lines if l.startswith("DIFF")]
    missing = [l for l in lines if l.startswith("MISSING")]
    assert len(missing) == 20 and all(re.search(r"^MISSING\s+-\s+\d+\s+_ZN4rtxo\d+(probe|shade|reference)_records_kernel", l) for l in missing), missing
    for unit in UNITS:
        assert unit + ".gfx950.s" in text, unit
    assert "new in this commit" in text
    for kernel in ("probe_kernel", "shade_tiles_kernel", "reference_tiles_kernel", "view_kernel", "accum_add_kernel"):
        assert kernel in text, kernel
    table = open(os.path.join(ROOT, "profiles", "rows_shade_isa_table.txt")).read()
    for kernel in RECORD_KERNELS | {"probe_kernel", "shade_tiles_kernel", "reference_tiles_kernel"}:
        assert kernel in table, kernel


# ---------------------------------------------------------------------------------------------- argument checks
def test_argument_checks_need_no_device(rtx, scene):
    """the byte twins' checks in the twins' order — NULLs and the light's cap, the frame and full width, no rows, the eye's
    range and the light's vertices, then the device — with a device number that does not exist, and the call's own: an unknown
    flag, d_shade's alignment, d_bytes"""
    L = rtx.rtx._lib
    h = scene.handle
    BAD, OK, UNSUPPORTED, NO_DEVICE = rtx.ERR_BAD_ARG, rtx.OK, rtx.ERR_UNSUPPORTED, rtx.ERR_NO_DEVICE
    rec = np.zeros(16 * 12, rtx.PIXEL_SHADE_DTYPE)
    rgb = np.zeros(16 * 12 * 3, np.uint8)
    own_light = scene.light()

    def host(view, light=None, flags=0, handle=h, out=rec.ctypes.data, stats=None, device=99):
        return L.rtx_render_view_rows_shade(handle, device, C.byref(view) if view is not None else None,
                                            C.byref(light) if light is not None else None, flags,
                                            C.cast(out, C.POINTER(rtx.rtx.PixelShade)), stats)

    def device(view, light=None, flags=0, handle=h, out=256, d_bytes=1 << 40, device=99):
        return L.rtx_render_view_rows_shade_device(handle, device, C.byref(view) if view is not None else None,
                                                   C.byref(light) if light is not None else None, flags, out, d_bytes, None, None)

    def twin_host(view, light, flags):
        if flags:
            return L.rtx_render_view_rows_posed(h, 99, C.byref(view), C.byref(light) if light is not None else None, rgb.ctypes.data, None)
        if light is None:
            return L.rtx_render_view_rows(h, 99, C.byref(view), rgb.ctypes.data, None)
        return L.rtx_render_view_rows_lit(h, 99, C.byref(view), C.byref(light), rgb.ctypes.data, None)

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
    for call in (host, device):
        for flags in (0, rtx.rtx.ROWS_POSED):
            for light in (None, own_light):
                assert call(own, light, flags, handle=None) == BAD and call(None, light, flags) == BAD and call(own, light, flags, out=None) == BAD
                assert call(own, light, flags) == NO_DEVICE == twin_host(own, light, flags)
                for v in (changed(x0=1), changed(nx=15), changed(nx=0), changed(nx=17), changed(y0=1), changed(ny=13),
                          changed(y0=0xFFFFFFF8, ny=12), changed(width=0, nx=0), changed(height=0, ny=0)):
                    assert call(v, light, flags) == BAD == twin_host(v, light, flags)
                for v in (far, changed(eye=(C.c_float * 3)(0.0, float("nan"), 0.0)), changed(eye=(C.c_float * 3)(0.0, 0.0, -10000.001))):
                    assert call(v, light, flags) == UNSUPPORTED == twin_host(v, light, flags)
                assert call(changed(eye=(C.c_float * 3)(10000.0, -10000.0, 10000.0)), light, flags) == NO_DEVICE
                assert call(changed(nx=15, eye=(C.c_float * 3)(3e4, 0.0, 0.0)), light, flags) == BAD
            assert call(own, light_with((1 << 20) + 1), flags) == BAD and call(own, light_with(1 << 20), flags) == NO_DEVICE
            assert call(own, light_with(0), flags) == NO_DEVICE
            for bad in (dict(v0=(float("nan"), 0.0, 0.0)), dict(v1=(0.0, float("inf"), 0.0)), dict(v2=(0.0, 0.0, float("-inf")))):
                assert call(own, light_with(9, **bad), flags) == UNSUPPORTED
            assert call(changed(nx=15), nan_light, flags) == BAD and call(far, nan_light, flags) == UNSUPPORTED
        # the call's own rule: a flag other than RTX_ROWS_POSED, whatever else holds
        for flags in (2, 3, 0x80000000, 0xFFFFFFFF):
            assert call(own, None, flags) == BAD and call(own, own_light, flags) == BAD and call(far, None, flags) == BAD
    # no rows: RTX_OK with the statistics zeroed, no device needed — whatever the eye
    st = rtx.rtx.Stats()
    st.primary_rays = 5
    assert host(changed(ny=0), stats=C.byref(st)) == OK and st.primary_rays == 0 and st.kernel_ms == 0.0
    assert host(changed(ny=0, y0=12)) == OK and host(changed(ny=0, eye=(C.c_float * 3)(3e4, 0.0, 0.0)), own_light) == OK
    assert device(changed(ny=0)) == OK and device(changed(ny=0), d_bytes=0) == OK
    # the device variant's buffer: 16-byte aligned, ny * width * 16 bytes at least, looked at before the eye and the device
    need = 12 * 16 * 16
    for light in (None, own_light):
        assert device(own, light, d_bytes=need) == NO_DEVICE and device(own, light, d_bytes=need - 1) == BAD
        assert device(far, light, d_bytes=need - 1) == BAD and device(far, light, d_bytes=need) == UNSUPPORTED
        assert device(changed(y0=3, ny=5), light, d_bytes=5 * 16 * 16) == NO_DEVICE
        assert device(changed(y0=3, ny=5), light, d_bytes=5 * 16 * 16 - 1) == BAD
        assert device(own, light, d_bytes=12 * 16 * 3) == BAD          # the byte twin's size is not enough
        for off in (1, 4, 8, 12, 15):
            assert device(own, light, out=256 + off) == BAD and device(far, light, out=256 + off) == BAD
        assert device(own, light, out=256 + 16) == NO_DEVICE
    with pytest.raises(rtx.RtxError) as e:
        scene.render_view_rows_shade(own, device=99)
    assert e.value.code == NO_DEVICE
