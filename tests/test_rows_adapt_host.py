"""The adaptive mean through the render pipeline without a GPU: the header, the exports and the bindings, where the masked
form of the scheduling pass lives in librtx.so, the unchanged ISA of every existing kernel, every argument check in the stated
order — each decided before a device is looked for — against rtx_render_view_adaptive's and rtx_render_view_rows_mean's
answers for the same arguments, and the empty rectangle."""
import ctypes as C
import importlib
import json
import os
import re
import subprocess

import numpy as np
import pytest

import accum_sets as ac
import light_sets as ls
import resample_sets as rs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FUNCS = ("rtx_render_view_rows_adaptive", "rtx_render_view_rows_adaptive_device", "rtx_render_view_rows_shade_masked_device")
METHODS = ("render_view_rows_adaptive", "render_view_rows_adaptive_device", "render_view_rows_shade_masked_device")
NOWHERE = 99                                # a device number no machine has: what is refused with it was refused on the host
D = 0x7F0000001000                          # a 16-byte aligned "device address": no call that is refused reads it
FORMS = {"probe_masked_kernelILb%dELb1ELb%dELb%dE" % (c, s, w) for c in (0, 1) for s in (0, 1) for w in (0, 1)}


@pytest.fixture(scope="module")
def rtx():
    return importlib.import_module("ray-tracer-rust_amd")


# ---------------------------------------------------------------------------------------------- header, exports, kernels
def test_header_declares_the_functions_and_the_library_exports_them(rtx):
    whole = open(os.path.join(ROOT, "include", "rtx.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", whole, flags=re.S)
    for f in FUNCS:
        assert re.search(r"\bint %s\s*\(" % f, hdr), f
    assert re.search(r"#define RTX_ABI_VERSION 3\b", hdr) and rtx.abi_version() == 3      # additions only
    flat = re.sub(r"\s+", " ", hdr)
    assert ("int rtx_render_view_rows_adaptive(RtxScene *scene, int device, const RtxView *view, const RtxLight *light , uint32_t flags , "
            "const uint64_t *seeds, uint32_t n_frames, uint32_t n_pairs, const RtxAdaptRule *rule, uint8_t *out_rgb, RtxPixelShade *out_shade, "
            "RtxTileState *out_tiles , RtxStats *stats);") in flat
    assert ("int rtx_render_view_rows_adaptive_device(RtxScene *scene, int device, const RtxView *view, const RtxLight *light, uint32_t flags , "
            "const uint64_t *seeds, uint32_t n_frames, uint32_t n_pairs, const RtxAdaptRule *rule, void *d_moments, void *d_tiles, void *d_rgb, "
            "void *d_shade, void *stream);") in flat
    assert ("int rtx_render_view_rows_shade_masked_device(RtxScene *scene, int device, const RtxView *view, const RtxLight *light, "
            "uint32_t flags , const void *d_tiles, const RtxAdaptRule *rule, void *d_shade, size_t d_bytes, void *stream, "
            "uint64_t *d_counters);") in flat
    said = re.sub(r"\s*\n \*\s*", " ", whole[whole.index("The adaptive mean through the render pipeline"):whole.index("int rtx_render_view_rows_adaptive(")])
    for words in ("word for word", "full width (RTX_ERR_BAD_ARG)", "RTX_ERR_UNSUPPORTED", "a first frame: the unmasked record launch",
                  "The aim kernels run once", "tiles row by row", "a descriptor that schedules nothing", "touches no counter",
                  "All n_frames frames are always enqueued", "The scene is not written", "keeps the words its records in d_shade held",
                  "adaptive motion blur", "not 8-byte aligned", "min_frames == 0", "negative or NaN"):
        assert words in said, words
    out = subprocess.check_output(["nm", "-D", "--defined-only", rtx.rtx.LIB_PATH], text=True)
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
    assert set(FUNCS) <= exported, set(FUNCS) - exported
    sigs = rtx.rtx._SIGS
    rs_text = open(os.path.join(ROOT, "integration", "rtx_ffi.rs")).read()
    block = re.search(r'extern "C" \{(.*?)\n\}', rs_text, re.S).group(1)
    layout = json.load(open(os.path.join(ROOT, "integration", "layout.json")))
    table = layout["rows_adapt"]
    P = C.POINTER
    ctype_of = {"scene": C.c_void_p, "u32": C.c_uint32, "i32": C.c_int, "u64*": rtx.rtx.u64p, "void*": C.c_void_p, "u8*": C.c_void_p,
                "usize": C.c_size_t, "shade*": P(rtx.rtx.PixelShade), "tile*": P(rtx.rtx.TileState), "rule*": P(rtx.rtx.AdaptRule),
                "view*": P(rtx.rtx.RtxView), "light*": P(rtx.rtx.RtxLight), "stats*": P(rtx.rtx.Stats)}
    ptr = r"\*(?:mut|const) "
    rust_of = {"scene": ptr + "RtxScene", "u32": "u32", "i32": "c_int", "u64*": ptr + "u64", "void*": ptr + "c_void", "u8*": ptr + "u8",
               "usize": "usize", "shade*": ptr + "RtxPixelShade", "tile*": ptr + "RtxTileState", "rule*": ptr + "RtxAdaptRule",
               "view*": ptr + "RtxView", "light*": ptr + "RtxLight", "stats*": ptr + "RtxStats"}
    assert set(table) == set(FUNCS)
    # the view-kernel calls' signatures, argument for argument
    assert table["rtx_render_view_rows_adaptive"] == layout["adapt"]["rtx_render_view_adaptive"]
    assert table["rtx_render_view_rows_adaptive_device"] == layout["adapt"]["rtx_render_view_adaptive_device"]
    for f in FUNCS:
        want = [ctype_of[t] for t in table[f]]
        if f.endswith("masked_device"):
            want[-1] = C.c_void_p                                        # (d_counters: a device address, as the unmasked call's binding)
            assert sigs[f][1][:-1] == sigs["rtx_render_view_rows_shade_device"][1][:5] + [C.c_void_p, P(rtx.rtx.AdaptRule)] + \
                sigs["rtx_render_view_rows_shade_device"][1][5:-1]
        assert sigs[f] == (C.c_int, want), f
        m = re.search(r"pub fn %s\((.*?)\) -> c_int;" % f, block, re.S)
        assert m, f
        args = [a.split(":")[1].strip() for a in m.group(1).split(",")]
        assert len(args) == len(table[f]) and all(re.fullmatch(rust_of[t], a) for t, a in zip(table[f], args)), (f, args)
    for meth in METHODS:
        assert callable(getattr(rtx.Scene, meth)), meth
    readme = open(os.path.join(ROOT, "README.md")).read()
    for name in FUNCS + ("tools/rows_adapt_timing.py", "rtxn"):
        assert name in readme, name
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in FUNCS:
        assert name in integration, name
    assert re.search(r"^## 27\. ", open(os.path.join(ROOT, "DESIGN.md")).read(), re.M)


def test_the_masked_forms_live_in_a_namespace_of_their_own():
    """librtx.so carries exactly the eight rtxn:: forms; rtx, rtxo, rtxe and rtxv hold what they held"""
    lib = os.path.join(ROOT, "ray-tracer-rust_amd", "librtx.so")
    blob = open(lib, "rb").read()

    def kernels(ns):
        return set(m.decode() for m in re.findall(rb"_ZN%d%s\d+([a-z0-9_]+_kernel(?:I(?:L[bij]\d+E)+)?)" % (len(ns), ns.encode()), blob)
                   if not m.startswith(b"__device_stub__"))

    assert kernels("rtxn") == FORMS, kernels("rtxn")
    records = {"probe_records_kernelILb%dELb1ELb%dELb%dE" % (c, s, w) for c in (0, 1) for s in (0, 1) for w in (0, 1)}
    shades = {"shade_records_kernelILb%dELb1ELi8ELb%dELb%dE" % (c, s, w) for c in (0, 1) for s in (0, 1) for w in (0, 1)}
    refs = {"reference_records_kernelILb%dELb%dE" % (c, s) for c in (0, 1) for s in (0, 1)}
    assert kernels("rtxo") == records | shades | refs, kernels("rtxo")
    assert kernels("rtxe") == {"view_masked_kernelILb0ELb0E", "view_masked_kernelILb0ELb1E", "view_masked_kernelILb1ELb0E",
                               "view_masked_kernelILb1ELb1E", "moment_add_kernel", "moment_resolve_kernel"}, kernels("rtxe")
    assert kernels("rtxv") == {"view_kernelILb0ELb0E", "view_kernelILb0ELb1E", "view_kernelILb1ELb0E", "view_kernelILb1ELb1E"}, kernels("rtxv")
    pipeline = kernels("rtx")
    assert {k.split("I")[0] for k in pipeline} == {"probe_kernel", "shade_tiles_kernel", "reference_tiles_kernel", "order_tiles_kernel",
                                                   "count_classes_kernel", "reset_kernel"}, pipeline
    assert len([k for k in pipeline if k.startswith("probe_kernel")]) == 12 and not any("masked" in k for k in pipeline)
    symbols = subprocess.run(["nm", "-C", lib], capture_output=True, text=True, check=True).stdout
    host_side = set(k for k in re.findall(r"\brtxn::(\w+_kernel)\b", symbols) if not k.startswith("__device_stub__"))
    assert host_side == {"probe_masked_kernel"}, host_side
    # the macro that makes them is set by rtx_kernel.hip alone
    csrc = os.path.join(ROOT, "ray-tracer-rust_amd", "csrc")
    assert "RTX_MASKED_FORMS" not in open(os.path.join(csrc, "Makefile")).read()
    kernel = open(os.path.join(csrc, "rtx_kernel.hip")).read()
    assert len(re.findall(r'^#include "rtx_pass_schedule\.hpp"', kernel, re.M)) == 3
    assert re.search(r"^namespace rtxn \{.*?#define RTX_RECORD_FORMS 1\n#define RTX_MASKED_FORMS 1[^\n]*\n#include \"rtx_pass_schedule\.hpp\"\n"
                     r"#undef RTX_MASKED_FORMS\n#undef RTX_RECORD_FORMS\n.*?^\}  // namespace rtxn", kernel, re.S | re.M)
    assert re.search(r"#if defined\(RTX_RECORD_FORMS\) \|\| defined\(RTX_MASKED_FORMS\)\n#error", kernel)


def test_existing_kernels_are_unchanged():
    """profiles/rows_adapt_same_isa.txt: tools/same_isa.py over `make asm` of the parent commit and of this one — every kernel
    of the parent SAME, and the only symbols without a counterpart are rtxn's eight"""
    text = open(os.path.join(ROOT, "profiles", "rows_adapt_same_isa.txt")).read()
    verdicts = re.findall(r"^\s*(SAME|DIFF|MISSING)\b", text, re.M)
    assert verdicts.count("SAME") >= 480 and "DIFF" not in verdicts, text
    for unit in ("rtx_kernel", "rtx_query", "rtx_shade", "rtx_view", "rtx_aim", "rtx_light", "rtx_tour", "rtx_pose", "rtx_planes",
                 "rtx_rebuild", "rtx_prims", "rtx_move", "rtx_skin", "rtx_samples", "rtx_accum", "rtx_adapt"):
        assert re.search(r"^%s\.gfx950\.s$" % unit, text, re.M), unit
    missing = re.findall(r"^\s*MISSING\s+(\S+)\s+(\S+)\s+(\S+)", text, re.M)
    assert len(missing) == 8 and all(a == "-" and b.isdigit() for a, b, _ in missing), missing      # in this commit only
    assert {re.match(r"_ZN4rtxn19(probe_masked_kernelILb\dELb\dELb\dELb\dE)", s).group(1) for _, _, s in missing} == FORMS
    for kernel in ("probe_kernel", "shade_tiles_kernel", "reference_tiles_kernel", "order_tiles_kernel", "moment_add_kernel",
                   "moment_resolve_kernel", "accum_add_kernel", "samples_kernel", "light_points_kernel", "tour_kernel"):
        assert re.search(r"^\s*SAME\b.*%s" % kernel, text, re.M), kernel
    for kernel, forms in (("_ZN4rtxo20probe_records_kernel", 8), ("_ZN4rtxo20shade_records_kernel", 8), ("_ZN4rtxo24reference_records_kernel", 4),
                          ("_ZN4rtxe18view_masked_kernel", 4), ("_ZN4rtxv11view_kernel", 4), ("_ZN3rtx12probe_kernel", 12)):
        assert len(re.findall(r"^\s*SAME\b.*%s" % kernel, text, re.M)) == forms, kernel
    table = open(os.path.join(ROOT, "profiles", "rows_adapt_isa_table.txt")).read()
    rows = re.findall(r"^(_ZN4rtx[no]\d+probe_(?:masked|records)_kernel\S+)\s+(\d+)\s+(\d+)\s+(\d+)\s+(\d+)\s+(\d+)\s+(\d+)\s+(\d+)$", table, re.M)
    assert len(rows) == 16 and all(r[3] == "0" and r[4] == "0" for r in rows)                      # no scratch, no vector spills


# ---------------------------------------------------------------------------------------------- argument checks
def test_adaptive_call_argument_checks_in_order(rtx, orc):
    """the adaptive call's own checks; then full width; then, on the host, the eye's range, the light, the frames' margins —
    beside rtx_render_view_adaptive's and rtx_render_view_rows_mean's answers for the same arguments"""
    L = rtx.rtx._lib
    BAD, NO_DEVICE, OK, UNSUPPORTED = rtx.ERR_BAD_ARG, rtx.ERR_NO_DEVICE, rtx.OK, rtx.ERR_UNSUPPORTED
    seeds = np.array(ac.SEEDS, np.uint64)
    sp = seeds.ctypes.data_as(rtx.rtx.u64p)
    good = rtx.rtx.AdaptRule(2, 1e-4)
    with rs.open_yard(rtx, ac.table(orc, 0)) as scene:
        h = scene.handle
        view = ac.yard_view(rtx)
        n = view.nx * view.ny
        rgb, shade, tiles = np.zeros((n, 3), np.uint8), np.zeros(n, rtx.PIXEL_SHADE_DTYPE), np.zeros(6, rtx.TILE_STATE_DTYPE)
        shp, tlp = shade.ctypes.data_as(C.POINTER(rtx.rtx.PixelShade)), tiles.ctypes.data_as(C.POINTER(rtx.rtx.TileState))
        light = rtx.Scene.make_light(*ls.SIDE_LIGHTS["far_side"])
        st = rtx.rtx.Stats()
        ref = lambda x: C.byref(x) if x is not None else None

        def host_of(fn, rule_arg=True):
            def call(scene_h=h, v=view, l=None, flags=0, s=sp, n_frames=3, n_pairs=ac.N_PAIRS, r=good, out_rgb=rgb.ctypes.data, out_shade=shp,
                     out_tiles=tlp, stats=None, dev=NOWHERE):
                head = (scene_h, dev, ref(v), ref(l), flags, s, n_frames, n_pairs)
                return fn(*head, ref(r), out_rgb, out_shade, out_tiles, stats) if rule_arg else fn(*head, out_rgb, out_shade, stats)
            return call

        def device_of(fn, rule_arg=True):
            def call(scene_h=h, v=view, l=None, flags=0, s=sp, n_frames=3, n_pairs=ac.N_PAIRS, r=good, mom=D, d_tiles=D + 0x8008,
                     d_rgb=D + 0x10001, d_shade=D + 0x20000, dev=NOWHERE):
                head = (scene_h, dev, ref(v), ref(l), flags, s, n_frames, n_pairs)
                return fn(*head, ref(r), mom, d_tiles, d_rgb, d_shade, None) if rule_arg else fn(*head, mom, d_rgb, d_shade, None)
            return call

        host, device = host_of(L.rtx_render_view_rows_adaptive), device_of(L.rtx_render_view_rows_adaptive_device)
        view_host, view_device = host_of(L.rtx_render_view_adaptive), device_of(L.rtx_render_view_adaptive_device)
        mean_host, mean_device = host_of(L.rtx_render_view_rows_mean, False), device_of(L.rtx_render_view_rows_mean_device, False)

        def altered(**fields):
            v = rtx.rtx.RtxView.from_buffer_copy(view)
            for k, x in fields.items():
                setattr(v, k, x)
            return v

        far = altered()
        far.eye[0] = 1e30                                               # an eye out of the pipeline's range
        nan_eye = altered()
        nan_eye.eye[2] = float("nan")
        wild = rtx.Scene.make_light(ls.SIDE_LIGHTS["far_side"][0], 7)
        wild.v1[1] = float("inf")
        huge = rtx.Scene.make_light(ls.SIDE_LIGHTS["far_side"][0], 7)   # finite vertices whose shaft margin is not: 3e38 + 3e38
        huge.v0[0], huge.v1[0] = 3e38, -3e38

        for call, twin, mean in ((host, view_host, mean_host), (device, view_device, mean_device)):
            assert call() == NO_DEVICE and call(l=light) == NO_DEVICE and call(n_frames=8, n_pairs=1) == NO_DEVICE
            # 1: the adaptive call's own checks, answered as the view-kernel call answers them
            cases = [dict(scene_h=None), dict(v=None), dict(s=None), dict(n_pairs=0), dict(r=None),
                     dict(l=rtx.Scene.make_light(ls.SIDE_LIGHTS["far_side"][0], 2 ** 20))]
            cases += [dict(n_frames=k) for k in (0, 65537, 0xFFFFFFFF)] + [dict(flags=f) for f in (4, 5, 0x80000000)]
            cases += [dict(r=rtx.rtx.AdaptRule(*bad)) for bad in ((0, 1e-4), (2, -1e-30), (2, float("nan")), (2, float("-inf")), (0, float("inf")))]
            cases += [dict(v=altered(**{f: x})) for f, x in (("width", 0), ("height", 0), ("y0", 10), ("ny", 17))]
            for kw in cases:
                assert call(**kw) == BAD == twin(**kw), kw
            for fine in ((1, 0.0), (2, float("inf")), (65536, 1e-4), (0xFFFFFFFF, 0.0)):
                assert call(r=rtx.rtx.AdaptRule(*fine)) == NO_DEVICE, fine
            assert call(flags=rtx.MEAN_POSED) == NO_DEVICE              # (no pose: decided on the device, as the mean does)
            # ... each ahead of full width, of the eye and of the light
            part = altered(x0=4, nx=16)
            for kw in (dict(r=None), dict(s=None), dict(n_frames=0), dict(flags=4)):
                assert call(v=part, **kw) == BAD and call(v=far, **kw) == BAD and call(l=wild, **kw) == BAD, kw
            # 2: full width: the view-kernel call takes the rectangle, the pipeline's calls do not — even for an eye out of
            # range or a wild light, and for an empty rectangle that is not full width
            for v in (part, altered(x0=1, nx=view.width - 1), altered(nx=view.width - 1), altered(x0=4, nx=16, ny=0), altered(nx=0)):
                assert call(v=v) == BAD == mean(v=v) and twin(v=v) in (NO_DEVICE, OK), (v.x0, v.nx, v.ny)
            far_part = altered(x0=4, nx=16)
            far_part.eye[0] = 1e30
            assert call(v=far_part) == BAD == mean(v=far_part) and call(v=part, l=wild) == BAD == mean(v=part, l=wild)
            # 3: decided on the host: the eye, the light, a frame's margin — where the view-kernel call goes on to look for a device
            for v in (far, nan_eye):
                assert call(v=v) == UNSUPPORTED == mean(v=v) and twin(v=v) == NO_DEVICE
            for bad in (np.nan, np.inf, -np.inf):
                w = rtx.Scene.make_light(ls.SIDE_LIGHTS["far_side"][0], 7)
                w.v1[1] = bad
                assert call(l=w) == UNSUPPORTED == mean(l=w) == twin(l=w), bad
            assert call(l=huge) == mean(l=huge) and call(l=huge) in (UNSUPPORTED, NO_DEVICE)
            # the empty rectangle: behind the rule and the width, ahead of the eye and the light; no device needed
            empty = altered(ny=0)
            assert call(v=empty) == OK == mean(v=empty) == twin(v=empty)
            assert call(v=empty, l=wild) == OK and call(v=empty, r=None) == BAD
            far_empty = altered(ny=0)
            far_empty.eye[0] = 1e30
            assert call(v=far_empty) == OK == mean(v=far_empty)
        # the variants' own
        assert host(out_rgb=None, out_shade=None) == BAD
        assert host(out_rgb=None) == NO_DEVICE and host(out_shade=None) == NO_DEVICE and host(out_tiles=None) == NO_DEVICE
        assert host(flags=rtx.ADAPT_CONTINUE) == BAD
        assert device(flags=rtx.ADAPT_CONTINUE) == NO_DEVICE and device(flags=rtx.ADAPT_CONTINUE | rtx.MEAN_POSED) == NO_DEVICE
        assert device(mom=None) == BAD and device(mom=D + 8) == BAD and device(d_shade=D + 0x20004) == BAD
        assert device(d_tiles=None) == BAD and device(d_tiles=D + 0x8004) == BAD and device(d_tiles=D + 0x8000) == NO_DEVICE
        assert device(d_rgb=None, d_shade=None) == NO_DEVICE            # the moments alone, for a later resolve
        for off in (0, 1, 2, 3):
            assert device(d_rgb=D + 0x10000 + off) == NO_DEVICE
        # the empty rectangle zeroes the statistics and writes nothing
        st.primary_rays = 77
        assert host(v=altered(ny=0), stats=C.byref(st)) == OK and st.primary_rays == 0 and st.kernel_ms == 0.0
        assert not rgb.any() and not shade["hits"].any() and not tiles["frames"].any()


def test_building_block_argument_checks(rtx, orc):
    """rtx_render_view_rows_shade_device's checks, answered as that call answers them, and the mask's own"""
    L = rtx.rtx._lib
    BAD, NO_DEVICE, OK, UNSUPPORTED = rtx.ERR_BAD_ARG, rtx.ERR_NO_DEVICE, rtx.OK, rtx.ERR_UNSUPPORTED
    good = rtx.rtx.AdaptRule(2, 1e-4)
    ref = lambda x: C.byref(x) if x is not None else None
    with rs.open_yard(rtx, ac.table(orc, 0)) as scene:
        h = scene.handle
        view = ac.yard_view(rtx)
        need = view.ny * view.width * 16

        def masked(scene_h=h, v=view, l=None, flags=0, d_tiles=D + 0x8008, r=good, d_shade=D, d_bytes=need, counters=None, dev=NOWHERE):
            return L.rtx_render_view_rows_shade_masked_device(scene_h, dev, ref(v), ref(l), flags, d_tiles, ref(r), d_shade, d_bytes, None, counters)

        def plain(scene_h=h, v=view, l=None, flags=0, d_shade=D, d_bytes=need, counters=None, dev=NOWHERE, **_):
            return L.rtx_render_view_rows_shade_device(scene_h, dev, ref(v), ref(l), flags, d_shade, d_bytes, None, counters)

        def altered(**fields):
            v = rtx.rtx.RtxView.from_buffer_copy(view)
            for k, x in fields.items():
                setattr(v, k, x)
            return v

        far = altered()
        far.eye[1] = -1e30
        wild = rtx.Scene.make_light(ls.SIDE_LIGHTS["far_side"][0], 7)
        wild.v2[0] = float("nan")
        assert masked() == NO_DEVICE == plain() and masked(counters=D + 0x40000) == NO_DEVICE
        assert masked(l=rtx.Scene.make_light(*ls.SIDE_LIGHTS["far_side"])) == NO_DEVICE and masked(flags=rtx.ROWS_POSED) == NO_DEVICE
        # the unmasked call's
        for kw in (dict(scene_h=None), dict(v=None), dict(d_shade=None), dict(d_shade=D + 8), dict(d_bytes=need - 1), dict(flags=2),
                   dict(flags=0x80000000), dict(v=altered(x0=4, nx=16)), dict(v=altered(nx=view.width - 1)), dict(v=altered(y0=10)),
                   dict(v=altered(width=0)), dict(l=rtx.Scene.make_light(ls.SIDE_LIGHTS["far_side"][0], 2 ** 20))):
            assert masked(**kw) == BAD == plain(**kw), kw
        for kw in (dict(v=far), dict(l=wild)):
            assert masked(**kw) == UNSUPPORTED == plain(**kw), kw
        assert masked(v=altered(ny=0), d_bytes=0) == OK == plain(v=altered(ny=0), d_bytes=0)
        # the mask's own: NULL or misaligned states, the rule
        assert masked(d_tiles=None) == BAD and masked(r=None) == BAD
        for off in (1, 2, 4, 12):
            assert masked(d_tiles=D + 0x8000 + off) == BAD, off
        assert masked(d_tiles=D + 0x8000) == NO_DEVICE
        for bad in ((0, 1e-4), (2, -1e-30), (2, float("nan")), (2, float("-inf")), (0, float("inf"))):
            assert masked(r=rtx.rtx.AdaptRule(*bad)) == BAD, bad
        for fine in ((1, 0.0), (2, float("inf")), (0xFFFFFFFF, 0.0)):
            assert masked(r=rtx.rtx.AdaptRule(*fine)) == NO_DEVICE, fine
        # ... and they hold for an empty rectangle and for an eye out of range too
        assert masked(v=altered(ny=0), d_tiles=None) == BAD and masked(v=far, r=None) == BAD and masked(v=far, d_tiles=D + 0x8004) == BAD
