"""Host side of the ray-query entry points (rtx_trace_rays, rtx_occluded_rays and their device-resident variants): the
header, the exported symbols, the layout of RtxRayHit in C, ctypes and the Rust binding, the argument checks that need no
device, and where the query kernels live in librtx.so's device code.  No GPU compute here."""
import ctypes as C
import importlib
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FUNCS = ("rtx_trace_rays", "rtx_occluded_rays", "rtx_trace_rays_device", "rtx_occluded_rays_device")
RENDER_KERNELS = {"reset_kernel", "probe_kernel", "count_classes_kernel", "order_tiles_kernel", "shade_tiles_kernel",
                  "reference_tiles_kernel"}


@pytest.fixture(scope="module")
def rtx():
    return importlib.import_module("ray-tracer-rust_amd")


@pytest.fixture(scope="module")
def scene(rtx, samples_half):
    tris, rgb = rtx.default_primitives([os.path.join(ROOT, "models", "bunny.obj")])
    with rtx.Scene(16, 16, tris, rgb, samples_half[:64], tie_rank=None) as s:
        yield s


def header():
    return open(os.path.join(ROOT, "include", "rtx.h")).read()


def test_header_declares_the_four_functions_and_the_library_exports_them(rtx):
    hdr = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)
    for f in FUNCS:
        assert re.search(r"\bint %s\s*\(" % f, hdr), f
    assert re.search(r"#define RTX_ABI_VERSION 3\b", hdr) and rtx.abi_version() == 3      # additions only
    assert re.search(r"#define RTX_NO_HIT 0xFFFFFFFFu", hdr) and re.search(r"#define RTX_RAYS_KEEP_ORDER\s+1u", hdr)
    out = subprocess.check_output(["nm", "-D", "--defined-only", rtx.rtx.LIB_PATH], text=True)
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
    assert set(FUNCS) <= exported, set(FUNCS) - exported
    assert set(FUNCS) <= set(rtx.rtx._SIGS)


def test_ray_hit_layout_in_c_ctypes_and_rust(rtx, tmp_path):
    src = tmp_path / "hit.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "rtx.h"\nint main(void) {\n'
                   'printf("%zu %zu %zu %zu %zu %zu\\n", sizeof(RtxRayHit), _Alignof(RtxRayHit), offsetof(RtxRayHit, prim),\n'
                   '       offsetof(RtxRayHit, t), offsetof(RtxRayHit, p_hit), offsetof(RtxRayHit, normal));\n'
                   'return (RTX_NO_HIT == 0xFFFFFFFFu && RTX_RAYS_KEEP_ORDER == 1u) ? 0 : 1; }\n')
    exe = tmp_path / "hit"
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    assert subprocess.check_output([str(exe)], text=True).split() == ["32", "4", "0", "4", "8", "20"]
    H = rtx.rtx.RayHit
    assert C.sizeof(H) == 32
    assert [(n, getattr(H, n).offset, getattr(H, n).size) for n, _ in H._fields_] == \
        [("prim", 0, 4), ("t", 4, 4), ("p_hit", 8, 12), ("normal", 20, 12)]
    dt = rtx.rtx.RAY_HIT_DTYPE
    assert dt.itemsize == 32 and [(n, dt.fields[n][1]) for n in dt.names] == [("prim", 0), ("t", 4), ("p_hit", 8), ("normal", 20)]
    rs = open(os.path.join(ROOT, "integration", "rtx_ffi.rs")).read()
    m = re.search(r"#\[repr\(C\)\]\s*(?:#\[derive\([^\)]*\)\]\s*)?pub struct RtxRayHit \{(.*?)\n\}", rs, re.S)
    assert m, "RtxRayHit with #[repr(C)] not found in rtx_ffi.rs"
    assert re.findall(r"pub (\w+): ([^,\n]+),", m.group(1)) == [("prim", "u32"), ("t", "f32"), ("p_hit", "[f32; 3]"),
                                                               ("normal", "[f32; 3]")]
    block = re.search(r'extern "C" \{(.*?)\n\}', rs, re.S).group(1)
    assert set(FUNCS) <= set(re.findall(r"pub fn (\w+)\(", block))


def test_bad_arguments_and_empty_batches_need_no_device(rtx, scene):
    L = rtx.rtx._lib
    f32p, u8p = rtx.rtx.f32p, rtx.rtx.u8p
    o = np.zeros((4, 3), np.float32)
    d = np.ones((4, 3), np.float32)
    hits = np.zeros(4, rtx.rtx.RAY_HIT_DTYPE)
    occ = np.zeros(4, np.uint8)
    op, dp = o.ctypes.data_as(f32p), d.ctypes.data_as(f32p)
    hp, cp = hits.ctypes.data_as(C.POINTER(rtx.rtx.RayHit)), occ.ctypes.data_as(u8p)
    h = scene.handle
    BAD, OK = rtx.ERR_BAD_ARG, rtx.OK
    # NULL pointers
    assert L.rtx_trace_rays(None, 0, 4, op, dp, 0, hp, None) == BAD
    assert L.rtx_trace_rays(h, 0, 4, None, dp, 0, hp, None) == BAD
    assert L.rtx_trace_rays(h, 0, 4, op, None, 0, hp, None) == BAD
    assert L.rtx_trace_rays(h, 0, 4, op, dp, 0, None, None) == BAD
    assert L.rtx_occluded_rays(None, 0, 4, op, dp, 0, cp, None) == BAD
    assert L.rtx_occluded_rays(h, 0, 4, None, dp, 0, cp, None) == BAD
    assert L.rtx_occluded_rays(h, 0, 4, op, None, 0, cp, None) == BAD
    assert L.rtx_occluded_rays(h, 0, 4, op, dp, 0, None, None) == BAD
    assert L.rtx_trace_rays_device(h, 0, 4, None, 256, 0, 512, None) == BAD
    assert L.rtx_trace_rays_device(h, 0, 4, 256, 512, 0, None, None) == BAD
    assert L.rtx_occluded_rays_device(h, 0, 4, 256, None, 0, 512, None) == BAD
    assert L.rtx_occluded_rays_device(None, 0, 4, 256, 512, 0, 768, None) == BAD
    # more than 2^28 rays, unknown flags, misaligned device pointers
    assert L.rtx_trace_rays(h, 0, (1 << 28) + 1, op, dp, 0, hp, None) == BAD
    assert L.rtx_occluded_rays(h, 0, (1 << 28) + 1, op, dp, 0, cp, None) == BAD
    assert L.rtx_trace_rays_device(h, 0, (1 << 28) + 1, 256, 512, 0, 768, None) == BAD
    assert L.rtx_trace_rays(h, 0, 4, op, dp, 4, hp, None) == BAD
    assert L.rtx_trace_rays_device(h, 0, 4, 256, 512, 0, 776, None) == BAD        # d_hits: 16-byte aligned
    assert L.rtx_trace_rays_device(h, 0, 4, 258, 512, 0, 768, None) == BAD
    # an empty batch is fine and writes nothing — also with no device at all, and whatever the flags
    hits["prim"] = 7
    occ[:] = 9
    st = rtx.rtx.Stats()
    st.primary_rays = 5
    assert L.rtx_trace_rays(h, 0, 0, op, dp, 0, hp, None) == OK
    assert L.rtx_trace_rays(h, 0, 0, op, dp, rtx.rtx.RAYS_KEEP_ORDER, hp, C.byref(st)) == OK
    assert st.primary_rays == 0 and st.rays == 0 and st.primary_hits == 0
    assert L.rtx_occluded_rays(h, 0, 0, op, dp, 0, cp, None) == OK
    assert L.rtx_trace_rays_device(h, 0, 0, 256, 512, 0, 768, None) == OK
    assert L.rtx_occluded_rays_device(h, 0, 0, 256, 512, 0, 769, None) == OK
    assert (hits["prim"] == 7).all() and (occ == 9).all()
    assert len(scene.trace_rays(np.zeros((0, 3)), np.zeros((0, 3)))) == 0
    with pytest.raises(ValueError):
        scene.trace_rays(o, d[:2])


def test_no_device_means_error_not_fallback(rtx, scene):
    if rtx.device_count() > 0:
        pytest.skip("a GPU is present")
    o = np.zeros((4, 3), np.float32)
    d = np.ones((4, 3), np.float32)
    for call in (lambda: scene.trace_rays(o, d), lambda: scene.occluded_rays(o, d), lambda: scene.trace_rays(o, d, keep_order=True),
                 lambda: scene.trace_rays_device(0, 4, 256, 512, 768), lambda: scene.occluded_rays_device(0, 4, 256, 512, 768)):
        with pytest.raises(rtx.RtxError) as e:
            call()
        assert e.value.code == rtx.ERR_NO_DEVICE


def test_query_kernels_live_in_their_own_namespace():
    """librtx.so carries the query kernels as rtxq::*_kernel, in every COUNT x SPHERES form, and its rtx:: kernels are
    still the render pipeline's six; it still imports no getenv (the radix sort it brings in included)."""
    lib = os.path.join(ROOT, "ray-tracer-rust_amd", "librtx.so")
    blob = open(lib, "rb").read()
    render = set(m.decode() for m in re.findall(rb"_ZN3rtx\d+([a-z0-9_]+_kernel)I?", blob) if not m.startswith(b"__device_stub__"))
    assert render == RENDER_KERNELS, render
    query = set(m.decode() for m in re.findall(rb"_ZN4rtxq\d+([a-z0-9_]+_kernel(?:ILb[01]ELb[01]E)?)", blob)
                if not m.startswith(b"__device_stub__"))
    forms = ["ILb%dELb%dE" % (c, s) for c in (0, 1) for s in (0, 1)]
    assert query == {"key_kernel"} | {"closest_kernel" + f for f in forms} | {"occluded_kernel" + f for f in forms}, query
    assert not re.search(rb"_ZN3rtx\d+[a-z0-9_]*(closest|occluded|key)_kernel", blob)
    undefined = subprocess.run(["nm", "-D", "--undefined-only", lib], capture_output=True, text=True, check=True).stdout
    assert "getenv" not in undefined
