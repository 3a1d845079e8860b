"""The adaptive mean of N frames without a GPU: the header, the exports and the bindings, the layouts of RtxMomentPixel,
RtxTileState and RtxAdaptRule, where the new kernels live in librtx.so, the unchanged ISA of the existing kernels, every
argument check — each decided before a device is looked for where the mean's is — RTX_ERR_NO_DEVICE for valid calls on a
device that does not exist, the host statements word for word against their numpy restatement on every fixture and against
the mean's host statements, and the sanitizer leg of the host side."""
import ctypes as C
import importlib
import json
import os
import re
import subprocess

import numpy as np
import pytest

import accum_sets as ac
import adapt_sets as ad
import light_sets as ls
import resample_sets as rs
from query_sets import F, bits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST_FUNCS = ("rtxh_moment_add", "rtxh_moment_resolve")
FUNCS = HOST_FUNCS + ("rtx_moment_add_device", "rtx_moment_resolve_device", "rtx_render_view_adaptive", "rtx_render_view_adaptive_device")
METHODS = ("render_view_adaptive", "render_view_adaptive_device", "moment_add_device", "moment_resolve_device")
STRUCTS = ("RtxMomentPixel", "RtxTileState", "RtxAdaptRule")
NOWHERE = 99                                # a device number no machine has: what is refused with it was refused on the host
D = 0x7F0000001000                          # a 16-byte aligned "device address": no call that is refused reads it


@pytest.fixture(scope="module")
def rtx():
    return importlib.import_module("ray-tracer-rust_amd")


@pytest.fixture(scope="module")
def thr(rtx, orc):
    with ac.open_bunny(rtx, ac.table(orc, 0)) as scene:
        return scene.gamma_thresholds()


# ---------------------------------------------------------------------------------------------- header, exports, kernels
def test_header_declares_the_functions_and_the_library_exports_them(rtx):
    whole = open(os.path.join(ROOT, "include", "rtx.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", whole, flags=re.S)
    for f in FUNCS:
        assert re.search(r"\bint %s\s*\(" % f, hdr), f
    assert re.search(r"#define RTX_ABI_VERSION 3\b", hdr) and rtx.abi_version() == 3      # additions only
    assert re.search(r"#define RTX_ADAPT_CONTINUE 2u\b", hdr) and rtx.ADAPT_CONTINUE == 2 and rtx.ADAPT_CONTINUE & rtx.MEAN_POSED == 0
    assert re.search(r"typedef struct RtxMomentPixel \{\s*float\s+sum\[3\];\s*uint32_t\s+hit_frames;\s*float\s+sumsq\[3\];\s*uint32_t\s+frames;\s*\} RtxMomentPixel;", hdr)
    assert re.search(r"typedef struct RtxTileState \{\s*uint32_t\s+frames;\s*float\s+err;\s*\} RtxTileState;", hdr)
    assert re.search(r"typedef struct RtxAdaptRule \{\s*uint32_t\s+min_frames;\s*float\s+max_variance;\s*\} RtxAdaptRule;", hdr)
    flat = re.sub(r"\s+", " ", hdr)
    assert ("int rtxh_moment_add(uint32_t nx, uint32_t ny, const RtxPixelShade *shade, RtxMomentPixel *moments, RtxTileState *tiles , "
            "uint32_t first, const RtxAdaptRule *rule );") in flat
    assert ("int rtx_moment_resolve_device(RtxScene *scene, int device, uint32_t n, const void *d_moments, void *d_rgb, void *d_shade, "
            "void *stream);") in flat
    said = re.sub(r"\s*\n \*\s*", " ", whole[whole.index("The adaptive mean of N frames: tiles stop"):whole.index("typedef struct RtxMomentPixel")])
    for words in ("THE STATEMENT", "never an FMA", "a < b ? b : a", "starting from +0.0", "there is no separate \"stopped\" word",
                  "stopping is final", "RTX_ADAPT_CONTINUE", "by the pixel's OWN count", "A TRAP", "min_frames >= 2 is the meaningful range",
                  "THE SCENE IS NOT WRITTEN", "more than 2^24 frames", "+infinity is allowed", "All n_frames frames are always enqueued",
                  "the sum over tiles of frames * pixels of the tile inside the rectangle * nb_ray"):
        assert words in said, words
    out = subprocess.check_output(["nm", "-D", "--defined-only", rtx.rtx.LIB_PATH], text=True)
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
    assert set(FUNCS) <= exported, set(FUNCS) - exported
    sigs = rtx.rtx._SIGS
    rs_text = open(os.path.join(ROOT, "integration", "rtx_ffi.rs")).read()
    block = re.search(r'extern "C" \{(.*?)\n\}', rs_text, re.S).group(1)
    table = json.load(open(os.path.join(ROOT, "integration", "layout.json")))["adapt"]
    P = C.POINTER
    ctype_of = {"scene": C.c_void_p, "f32*": rtx.rtx.f32p, "u32": C.c_uint32, "i32": C.c_int, "u64*": rtx.rtx.u64p, "void*": C.c_void_p,
                "u8*": C.c_void_p, "shade*": P(rtx.rtx.PixelShade), "moment*": P(rtx.rtx.MomentPixel), "tile*": P(rtx.rtx.TileState),
                "rule*": P(rtx.rtx.AdaptRule), "view*": P(rtx.rtx.RtxView), "light*": P(rtx.rtx.RtxLight), "stats*": P(rtx.rtx.Stats)}
    ptr = r"\*(?:mut|const) "
    rust_of = {"scene": ptr + "RtxScene", "f32*": ptr + "f32", "u32": "u32", "i32": "c_int", "u64*": ptr + "u64", "void*": ptr + "c_void",
               "u8*": ptr + "u8", "shade*": ptr + "RtxPixelShade", "moment*": ptr + "RtxMomentPixel", "tile*": ptr + "RtxTileState",
               "rule*": ptr + "RtxAdaptRule", "view*": ptr + "RtxView", "light*": ptr + "RtxLight", "stats*": ptr + "RtxStats"}
    assert set(k for k in table if not k.startswith(STRUCTS)) == set(FUNCS)
    for f in FUNCS:
        assert sigs[f] == (C.c_int, [ctype_of[t] for t in table[f]]), f
        m = re.search(r"pub fn %s\((.*?)\) -> c_int;" % f, block, re.S)
        assert m, f
        args = [a.split(":")[1].strip() for a in m.group(1).split(",")]
        assert len(args) == len(table[f]) and all(re.fullmatch(rust_of[t], a) for t, a in zip(table[f], args)), (f, args)
    assert re.search(r"pub const RTX_ADAPT_CONTINUE: u32 = 2;", rs_text)
    for meth in METHODS:
        assert callable(getattr(rtx.Scene, meth)), meth
    assert callable(rtx.moment_add) and callable(rtx.moment_resolve)
    readme = open(os.path.join(ROOT, "README.md")).read()
    for name in FUNCS + ("rtx_adapt.hip", "rtx_adapt.h", "tools/adapt_timing.py"):
        assert name in readme, name
    assert re.search(r"^## 26\. ", open(os.path.join(ROOT, "DESIGN.md")).read(), re.M)
    mk = open(os.path.join(ROOT, "ray-tracer-rust_amd", "csrc", "Makefile")).read()
    assert re.search(r"^UNITS\s*:=.*\brtx_adapt\b", mk, re.M) and "rtx_adapt.h" in mk             # the library and `make asm`


def test_the_three_structs_have_the_stated_layout(rtx):
    table = json.load(open(os.path.join(ROOT, "integration", "layout.json")))["adapt"]
    rs_text = open(os.path.join(ROOT, "integration", "rtx_ffi.rs")).read()
    rust_type = {"sum": r"\[f32; 3\]", "sumsq": r"\[f32; 3\]", "err": "f32", "max_variance": "f32"}
    for name, ctype, dtype in (("RtxMomentPixel", rtx.rtx.MomentPixel, rtx.MOMENT_PIXEL_DTYPE), ("RtxTileState", rtx.rtx.TileState, rtx.TILE_STATE_DTYPE),
                               ("RtxAdaptRule", rtx.rtx.AdaptRule, None)):
        assert table[name] == [C.sizeof(ctype), C.alignment(ctype)], name
        fields = [f for f, _ in ctype._fields_]
        assert [k.split(".")[1] for k in table if k.startswith(name + ".")] == fields
        for f in fields:
            d = getattr(ctype, f)
            assert table["%s.%s" % (name, f)] == [d.offset, d.size], (name, f)
            if dtype is not None:
                assert dtype.fields[f][1] == d.offset and dtype.fields[f][0].itemsize == d.size, (name, f)
        body = r"\s*".join(r"pub %s: %s," % (f, rust_type.get(f, "u32")) for f in fields)
        assert re.search(r"#\[repr\(C\)\]\s*#\[derive\([^)]*\)\]\s*pub struct %s \{\s*%s\s*\}" % (name, body), rs_text), name
    assert table["RtxMomentPixel"][0] == 32 and table["RtxTileState"][0] == 8 and table["RtxAdaptRule"][0] == 8
    # gcc's layout of the header itself
    src = "#include <stddef.h>\n#include <stdio.h>\n#include \"rtx.h\"\nint main(void){printf(\"%zu %zu %zu %zu %zu %zu %zu %zu\\n\"," \
          "sizeof(RtxMomentPixel),offsetof(RtxMomentPixel,hit_frames),offsetof(RtxMomentPixel,sumsq),offsetof(RtxMomentPixel,frames)," \
          "sizeof(RtxTileState),offsetof(RtxTileState,err),sizeof(RtxAdaptRule),offsetof(RtxAdaptRule,max_variance));return 0;}\n"
    import tempfile
    with tempfile.TemporaryDirectory() as tmp:
        open(os.path.join(tmp, "l.c"), "w").write(src)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), os.path.join(tmp, "l.c"), "-o", os.path.join(tmp, "l")])
        assert subprocess.check_output([os.path.join(tmp, "l")], text=True).split() == ["32", "12", "16", "28", "8", "4", "8", "4"]


def test_the_new_kernels_live_in_their_own_namespace():
    """librtx.so carries exactly the rtxe:: kernels; the sets of rtxv, rtxc and the other small units are what they were"""
    lib = os.path.join(ROOT, "ray-tracer-rust_amd", "librtx.so")
    blob = open(lib, "rb").read()

    def kernels(ns):
        return set(m.decode() for m in re.findall(rb"_ZN%d%s\d+([a-z0-9_]+_kernel(?:ILb[01]ELb[01]E)?)" % (len(ns), ns.encode()), blob)
                   if not m.startswith(b"__device_stub__"))

    assert kernels("rtxe") == {"view_masked_kernelILb0ELb0E", "view_masked_kernelILb0ELb1E", "view_masked_kernelILb1ELb0E",
                               "view_masked_kernelILb1ELb1E", "moment_add_kernel", "moment_resolve_kernel"}, kernels("rtxe")
    assert kernels("rtxv") == {"view_kernelILb0ELb0E", "view_kernelILb0ELb1E", "view_kernelILb1ELb0E", "view_kernelILb1ELb1E"}, kernels("rtxv")
    assert kernels("rtxc") == {"accum_add_kernel", "accum_resolve_kernel"}, kernels("rtxc")
    assert kernels("rtxr") == {"samples_kernel"} and kernels("rtxl") == {"light_points_kernel"} and kernels("rtxk") == {"skin_kernel"}
    symbols = subprocess.run(["nm", "-C", lib], capture_output=True, text=True, check=True).stdout
    host_side = set(k for k in re.findall(r"\brtxe::(\w+_kernel)\b", symbols) if not k.startswith("__device_stub__"))
    assert host_side == {"view_masked_kernel", "moment_add_kernel", "moment_resolve_kernel"}, host_side


def test_existing_kernels_are_unchanged():
    """profiles/adapt_same_isa.txt: tools/same_isa.py over `make asm` of the parent commit and of this one, every existing
    unit — one SAME line per kernel and no other verdict"""
    text = open(os.path.join(ROOT, "profiles", "adapt_same_isa.txt")).read()
    verdicts = re.findall(r"^\s*(SAME|DIFF|MISSING)\b", text, re.M)
    assert len(verdicts) >= 20 and set(verdicts) == {"SAME"}, text
    for unit in ("rtx_kernel", "rtx_query", "rtx_shade", "rtx_view", "rtx_aim", "rtx_light", "rtx_tour", "rtx_pose", "rtx_planes",
                 "rtx_rebuild", "rtx_prims", "rtx_move", "rtx_skin", "rtx_samples", "rtx_accum"):
        assert re.search(r"^%s\.gfx950\.s$" % unit, text, re.M), unit
    for kernel in ("samples_kernel", "skin_kernel", "move_kernel", "overlay_kernel", "pose_records_kernel", "light_points_kernel",
                   "tour_kernel", "probe_kernel", "shade_tiles_kernel", "accum_add_kernel", "accum_resolve_kernel"):
        assert re.search(r"^\s*SAME\b.*%s" % kernel, text, re.M), kernel
    assert len(re.findall(r"^\s*SAME\b.*_ZN4rtxv11view_kernelILb[01]ELb[01]E", text, re.M)) == 4          # the four forms
    assert not re.search(r"^\s*\w+\s.*(moment_add_kernel|moment_resolve_kernel|view_masked_kernel)", text, re.M)   # no counterpart


# ---------------------------------------------------------------------------------------------- argument checks
def test_building_block_argument_checks(rtx, orc):
    L = rtx.rtx._lib
    BAD, NO_DEVICE, OK = rtx.ERR_BAD_ARG, rtx.ERR_NO_DEVICE, rtx.OK
    rule = rtx.rtx.AdaptRule(2, 0.5)
    rp = C.byref(rule)
    with ac.open_bunny(rtx, ac.table(orc, 0)) as scene:
        h = scene.handle
        for dev in (NOWHERE, 0):
            add = lambda s=h, nx=5, ny=3, shade=D, mom=D + 0x1000, tiles=D + 0x2000, first=0, r=rp: \
                L.rtx_moment_add_device(s, dev, nx, ny, shade, mom, tiles, first, r, None)
            assert add(s=None) == BAD and add(shade=None) == BAD and add(mom=None) == BAD and add(r=None) == BAD
            for off in (1, 2, 4, 8, 12):
                assert add(shade=D + off) == BAD and add(mom=D + 0x1000 + off) == BAD, off
            for off in (1, 2, 4, 12):
                assert add(tiles=D + 0x2000 + off) == BAD, off
            for bad in ((0, 0.5), (2, -1.0), (2, float("nan")), (2, float("-inf")), (0, float("inf"))):
                assert add(r=C.byref(rtx.rtx.AdaptRule(*bad))) == BAD, bad
            assert add(nx=1 << 14, ny=(1 << 14) + 1) == BAD
            # ... and they are checked for an empty rectangle too; a valid call of no records is RTX_OK with no device
            assert add(nx=0, mom=D + 4) == BAD and add(ny=0, r=None) == BAD
            assert add(nx=0) == OK and add(ny=0, first=1) == OK and add(nx=0, tiles=None, r=None) == OK
            assert add(nx=0, tiles=D + 0x2008, r=C.byref(rtx.rtx.AdaptRule(1, float("inf")))) == OK         # 8-byte aligned; +infinity
            res = lambda s=h, n=4, mom=D, rgb=D + 0x1001, shade=D + 0x2000: L.rtx_moment_resolve_device(s, dev, n, mom, rgb, shade, None)
            assert res(s=None) == BAD and res(mom=None) == BAD and res(rgb=None, shade=None) == BAD
            for off in (1, 2, 4, 8):
                assert res(mom=D + off) == BAD and res(shade=D + 0x2000 + off) == BAD, off
            assert res(n=0, mom=D + 8) == BAD
            for off in (0, 1, 2, 3):                                    # d_rgb may have any alignment
                assert res(n=0, rgb=D + 0x1000 + off, shade=None) == OK, off
        # valid calls on a device that does not exist
        assert L.rtx_moment_add_device(h, NOWHERE, 5, 3, D, D + 0x1000, D + 0x2000, 0, rp, None) == NO_DEVICE
        assert L.rtx_moment_add_device(h, -1, 5, 3, D, D + 0x1000, None, 1, None, None) == NO_DEVICE
        assert L.rtx_moment_resolve_device(h, NOWHERE, 4, D, D + 0x1003, None, None) == NO_DEVICE
        assert L.rtx_moment_resolve_device(h, NOWHERE, 4, D, None, D + 0x2000, None) == NO_DEVICE
    # the host statements
    shade, mom, tiles = np.zeros((3, 5), rtx.PIXEL_SHADE_DTYPE), np.zeros((3, 5), rtx.MOMENT_PIXEL_DTYPE), np.zeros((1, 1), rtx.TILE_STATE_DTYPE)
    sp, mp, tp = (a.ctypes.data_as(C.POINTER(t)) for a, t in ((shade, rtx.rtx.PixelShade), (mom, rtx.rtx.MomentPixel), (tiles, rtx.rtx.TileState)))
    thr, rgb = np.zeros(256, np.float32), np.zeros(45, np.uint8)
    fp = thr.ctypes.data_as(rtx.rtx.f32p)
    assert L.rtxh_moment_add(5, 3, None, mp, tp, 0, rp) == BAD and L.rtxh_moment_add(5, 3, sp, None, tp, 1, rp) == BAD
    assert L.rtxh_moment_add(5, 3, sp, mp, tp, 1, None) == BAD and L.rtxh_moment_add(1 << 14, (1 << 14) + 1, sp, mp, None, 1, None) == BAD
    for bad in ((0, 0.5), (2, -1.0), (2, float("nan"))):
        assert L.rtxh_moment_add(5, 3, sp, mp, tp, 1, C.byref(rtx.rtx.AdaptRule(*bad))) == BAD, bad
    assert L.rtxh_moment_add(0, 3, sp, mp, tp, 0, rp) == OK and L.rtxh_moment_add(5, 0, sp, mp, None, 0, None) == OK and not mom["frames"].any()
    assert L.rtxh_moment_add(5, 3, sp, mp, None, 1, None) == OK and (mom["frames"] == 1).all() and not tiles["frames"].any()
    assert L.rtxh_moment_resolve(None, 15, mp, rgb.ctypes.data, sp) == BAD and L.rtxh_moment_resolve(fp, 15, None, rgb.ctypes.data, sp) == BAD
    assert L.rtxh_moment_resolve(fp, 15, mp, None, None) == BAD
    assert L.rtxh_moment_resolve(fp, 15, mp, rgb.ctypes.data, None) == OK and L.rtxh_moment_resolve(fp, 0, mp, None, sp) == OK


def test_adaptive_call_argument_checks(rtx, orc):
    """the adaptive call's own checks and the mean's, every one decided before a device is looked for; then the mean's
    order: the empty rectangle, the light that is not finite, the device"""
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

        def host(scene_h=h, v=view, l=None, flags=0, s=sp, n_frames=3, n_pairs=ac.N_PAIRS, r=good, out_rgb=rgb.ctypes.data, out_shade=shp,
                 out_tiles=tlp, stats=None, dev=NOWHERE):
            return L.rtx_render_view_adaptive(scene_h, dev, ref(v), ref(l), flags, s, n_frames, n_pairs, ref(r), out_rgb, out_shade, out_tiles, stats)

        def device(scene_h=h, v=view, l=None, flags=0, s=sp, n_frames=3, n_pairs=ac.N_PAIRS, r=good, mom=D, d_tiles=D + 0x8008, d_rgb=D + 0x10001,
                   d_shade=D + 0x20000, dev=NOWHERE):
            return L.rtx_render_view_adaptive_device(scene_h, dev, ref(v), ref(l), flags, s, n_frames, n_pairs, ref(r), mom, d_tiles, d_rgb, d_shade, None)

        for call in (host, device):
            assert call() == NO_DEVICE and call(l=light) == NO_DEVICE and call(n_frames=8, n_pairs=1) == NO_DEVICE
            assert call(scene_h=None) == BAD and call(v=None) == BAD and call(s=None) == BAD
            for n_frames in (0, 65537, 0xFFFFFFFF):
                assert call(n_frames=n_frames) == BAD, n_frames
            assert call(n_pairs=0) == BAD
            for flags in (4, 5, 0x80000000):
                assert call(flags=flags) == BAD, flags
            assert call(flags=rtx.MEAN_POSED) == NO_DEVICE              # (no pose: decided on the device, as the mean does)
            # the rule: NULL, min_frames == 0, a negative or NaN threshold; +infinity and 0 are allowed
            assert call(r=None) == BAD
            for bad in ((0, 1e-4), (2, -1e-30), (2, float("nan")), (2, float("-inf")), (0, float("inf"))):
                assert call(r=rtx.rtx.AdaptRule(*bad)) == BAD, bad
            for fine in ((1, 0.0), (2, float("inf")), (65536, 1e-4), (0xFFFFFFFF, 0.0)):
                assert call(r=rtx.rtx.AdaptRule(*fine)) == NO_DEVICE, fine
            # the mean's view checks
            for field, value in (("width", 0), ("height", 0), ("x0", 20), ("y0", 10), ("nx", 25), ("ny", 17)):
                v = rtx.rtx.RtxView.from_buffer_copy(view)
                setattr(v, field, value)
                assert call(v=v) == BAD, field
            # the mean's light checks: more than 2^20 points; a vertex that is not finite is UNSUPPORTED, on the host
            assert call(l=rtx.Scene.make_light(ls.SIDE_LIGHTS["far_side"][0], 2 ** 20)) == BAD
            for bad in (np.nan, np.inf, -np.inf):
                wild = rtx.Scene.make_light(ls.SIDE_LIGHTS["far_side"][0], 7)
                wild.v1[1] = bad
                assert call(l=wild) == UNSUPPORTED, bad
                # ... behind the empty rectangle, which needs no device and writes nothing
                for field in ("nx", "ny"):
                    v = rtx.rtx.RtxView.from_buffer_copy(view)
                    setattr(v, field, 0)
                    assert call(v=v, l=wild) == OK and call(v=v) == OK
                    assert call(v=v, r=None) == BAD                     # ... but not before the rule
        # the variants' own: both outputs NULL (host; the tile states alone are no output); RTX_ADAPT_CONTINUE is the device
        # variant's; NULL or misaligned moments, tile states or records (d_rgb: any alignment)
        assert host(out_rgb=None, out_shade=None) == BAD
        assert host(out_rgb=None) == NO_DEVICE and host(out_shade=None) == NO_DEVICE and host(out_tiles=None) == NO_DEVICE
        assert host(flags=rtx.ADAPT_CONTINUE) == BAD
        assert device(flags=rtx.ADAPT_CONTINUE) == NO_DEVICE and device(flags=rtx.ADAPT_CONTINUE | rtx.MEAN_POSED) == NO_DEVICE
        assert device(mom=None) == BAD and device(mom=D + 8) == BAD and device(d_shade=D + 0x20004) == BAD
        assert device(d_tiles=None) == BAD and device(d_tiles=D + 0x8004) == BAD and device(d_tiles=D + 0x8000) == NO_DEVICE
        assert device(d_rgb=None, d_shade=None) == NO_DEVICE            # the moments alone, for a later resolve
        for off in (0, 1, 2, 3):
            assert device(d_rgb=D + 0x10000 + off) == NO_DEVICE
        # the empty rectangle zeroes the statistics
        v = rtx.rtx.RtxView.from_buffer_copy(view)
        v.nx = 0
        st.primary_rays = 77
        assert host(v=v, stats=C.byref(st)) == OK and st.primary_rays == 0 and st.kernel_ms == 0.0
        assert not rgb.any() and not shade["hits"].any() and not tiles["frames"].any()


# ---------------------------------------------------------------------------------------------- the host statements
def host_run(rtx, rule, records, state=None):
    """the frames through rtxh_moment_add -> (moments, tiles, the tile states after every frame)"""
    history = []
    mom, tiles = state if state else (None, None)
    for rec in records:
        mom, tiles = rtx.moment_add(rec, mom, tiles, rule=rule)
        history.append(tiles.copy())
    return mom, tiles, history


@pytest.mark.parametrize("fixture", ("bunny", "ragged", "ragged_low", "yard", "yard_posed"))
def test_host_statements_give_the_fixtures_expected_values(orc, rtx, thr, fixture):
    e = ad.expected(orc, rtx, fixture)
    lins, hits = ad.fixture_frames(orc, rtx, fixture, ad.fixture_count(fixture))
    records = [ac.as_records(rtx, lin, np.zeros(lin.shape, np.uint8), hit.astype(np.uint8)) for lin, hit in zip(lins, hits)]
    mom, tiles, history = host_run(rtx, ad.fixture_rule(fixture), records)
    assert ad.same_moments(mom, e["mom"]) and ad.same_tiles(tiles, e["tiles"])
    for k, (got, want) in enumerate(zip(history, e["history"])):
        assert ad.same_tiles(got, want), (fixture, k)
    rgb, shade = rtx.moment_resolve(thr, mom)
    assert ac.same_records(shade, ac.as_records(rtx, e["linear"], e["rgb8"], e["hits"])) and np.array_equal(rgb, e["rgb8"])
    assert ac.same_records(shade, ad.np_resolve(rtx, thr, e["mom"]))


def test_host_statements_on_the_synthetic_records(rtx, thr):
    syn = ad.synthetic(rtx)
    ny, nx = ad.SYNTHETIC_SHAPE
    # first over moments and tile states of 0xAA bytes: bit for bit, a NaN's payload included; the old content is not read
    mom = np.frombuffer(bytes([0xAA]) * (32 * nx * ny), rtx.MOMENT_PIXEL_DTYPE).copy().reshape(ny, nx)
    tiles = np.frombuffer(bytes([0xAA]) * (8 * 20), rtx.TILE_STATE_DTYPE).copy().reshape(4, 5)
    rule = rtx.rtx.AdaptRule(*ad.SYNTHETIC_RULE)
    assert rtx.rtx._lib.rtxh_moment_add(nx, ny, syn[0].ctypes.data_as(C.POINTER(rtx.rtx.PixelShade)), mom.ctypes.data_as(C.POINTER(rtx.rtx.MomentPixel)),
                                        tiles.ctypes.data_as(C.POINTER(rtx.rtx.TileState)), 1, C.byref(rule)) == rtx.OK
    assert np.array_equal(bits(mom["sum"]), bits(syn[0]["linear"])) and (mom["frames"] == 1).all() and (tiles["frames"] == 1).all()
    assert (bits(tiles["err"]) == 0).all()                              # one frame: the variance is exactly +0, NaN records included
    for rule in (ad.SYNTHETIC_RULE, (3, float("inf")), (2, 1.0), (1, 0.0)):
        for n in range(1, ac.SYNTHETIC_FRAMES + 1):
            e = ad.synthetic_run(rtx, rule, n)
            mom, tiles, history = host_run(rtx, rule, syn[:n])
            assert ad.same_moments(mom, e["mom"]) and ad.same_tiles(tiles, e["tiles"]), (rule, n)
            assert not np.isnan(tiles["err"]).any() and (tiles["err"] >= 0).all()
            rgb, shade = rtx.moment_resolve(thr, mom)
            want = ad.np_resolve(rtx, thr, e["mom"])
            assert ac.same_records(shade, want) and np.array_equal(rgb, want["rgb8"]), (rule, n)
    # without tile states: the plain moment accumulator, whose sum and hit_frames are the mean's accumulator
    mom = acc = None
    for rec in syn:
        mom = rtx.moment_add(rec, mom)
        acc = rtx.accum_add(rec, acc)
    e = ad.synthetic_run(rtx, (ac.SYNTHETIC_FRAMES, 0.0))
    assert ad.same_moments(mom, e["mom"]) and ac.same_accum(acc, mom["sum"], mom["hit_frames"])


@pytest.mark.parametrize("fixture,n", (("bunny", 1), ("bunny", 3), ("bunny", 8), ("yard", 3)))
def test_with_min_frames_of_n_the_words_are_the_means(orc, rtx, thr, fixture, n):
    lins, hits = ad.fixture_frames(orc, rtx, fixture, n)
    records = [ac.as_records(rtx, lin, np.zeros(lin.shape, np.uint8), hit.astype(np.uint8)) for lin, hit in zip(lins, hits)]
    mom, tiles, _ = host_run(rtx, (n, 0.0), records)
    acc = None
    for rec in records:
        acc = rtx.accum_add(rec, acc)
    assert np.array_equal(bits(mom["sum"]), bits(acc["sum"])) and np.array_equal(mom["hit_frames"], acc["hit_frames"])
    assert (mom["frames"] == n).all() and (tiles["frames"] == n).all()
    rgb, shade = rtx.moment_resolve(thr, mom)
    m_rgb, m_shade = rtx.accum_resolve(thr, acc, n)
    assert shade.tobytes() == m_shade.tobytes() and np.array_equal(rgb, m_rgb)


def test_continue_and_a_stricter_rule_on_the_host(orc, rtx):
    """3 + 5 frames are 8; a continued run under a stricter rule resumes stopped tiles by itself"""
    lins, hits = ad.fixture_frames(orc, rtx, "bunny", ad.N_FRAMES)
    records = [ac.as_records(rtx, lin, np.zeros(lin.shape, np.uint8), hit.astype(np.uint8)) for lin, hit in zip(lins, hits)]
    e = ad.expected(orc, rtx, "bunny")
    mom, tiles, _ = host_run(rtx, ad.RULE, records[:3])
    mom, tiles, _ = host_run(rtx, ad.RULE, records[3:], (mom, tiles))
    assert ad.same_moments(mom, e["mom"]) and ad.same_tiles(tiles, e["tiles"])
    strict = (2, float(F(3e-7)))
    mom, tiles, _ = host_run(rtx, ad.RULE, records[:4])
    before = tiles.copy()
    mom, tiles, _ = host_run(rtx, strict, records[4:], (mom, tiles))
    first = ad.run(ad.RULE, lins[:4], hits[:4])
    want = ad.run(strict, lins[4:], hits[4:], state=(first["mom"], first["tiles"]))
    assert ad.same_moments(mom, want["mom"]) and ad.same_tiles(tiles, want["tiles"])
    resumed = ad.np_stopped(ad.RULE, before) & (tiles["frames"] > before["frames"])
    assert resumed.sum() >= 2 and (ad.np_stopped(ad.RULE, before) & ~resumed).sum() >= 2


# ---------------------------------------------------------------------------------------------- sanitizers
def test_host_side_is_clean_under_asan_and_ubsan(tmp_path):
    out = subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "tests", "sanitize_adapt"), "run", "OUT=%s" % tmp_path],
                         capture_output=True, text=True, timeout=900)
    text = out.stdout + out.stderr
    assert out.returncode == 0, text[-4000:]
    assert "adapt sanitizer driver: 0 failed checks" in text
    assert "ERROR: AddressSanitizer" not in text and "runtime error" not in text and "LeakSanitizer" not in text, text[-4000:]
