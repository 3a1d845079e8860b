"""rtx_shade_rays without a GPU: the test helper shade_sets.oracle_shade pinned against the oracle's own render_pixel, the
conditions the ray sets must meet to test what they are for, the layout of RtxPixelShade in C, ctypes, numpy and the Rust
binding, the exported functions, the argument checks that need no device, and where the kernels live in librtx.so."""
import ctypes as C
import importlib
import os
import re
import subprocess

import numpy as np
import pytest

import query_sets as qs
import shade_sets as ss
from query_sets import F, H, NO_HIT, W, bits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FUNCS = ("rtx_shade_rays", "rtx_shade_rays_device")


@pytest.fixture(scope="module")
def rtx():
    return importlib.import_module("ray-tracer-rust_amd")


@pytest.fixture(scope="module")
def bunny(orc, samples_seeded):
    return ss.bunny_sets(orc, samples_seeded)


@pytest.fixture(scope="module")
def soup(orc, samples_seeded):
    return ss.soup_sets(orc, samples_seeded)


@pytest.fixture(scope="module")
def scene(rtx, samples_half):
    tris, rgb = rtx.default_primitives([os.path.join(ROOT, "models", "bunny.obj")])
    with rtx.Scene(16, 16, tris, rgb, samples_half[:64], tie_rank=None) as s:
        yield s


# ---------------------------------------------------------------------------------------------- the helper is render_pixel
def check_against_render_rows(orc, osc, s, px, py, nb_ray, samples, cam, distance, eye):
    """Ray::new of the raw directions is create_ray's direction, bit for bit; oracle_shade on those rays is the oracle's
    render_pixel: linear colour, bytes"""
    L = orc.lib()
    u, v, w = cam
    o, d = np.zeros(3, F), np.zeros(3, F)
    for k in range(len(px)):
        for i in range(nb_ray):
            L.orc_create_ray(int(px[k]), int(py[k]), i, osc.width, osc.height, orc._fp(orc.f3(eye)), orc._fp(u), orc._fp(v),
                             orc._fp(w), float(distance), orc._fp(samples), len(samples), orc._fp(o), orc._fp(d))
            assert bits(s["units"][k * nb_ray + i]).tolist() == bits(d).tolist(), (k, i)
            assert bits(s["origins"][k * nb_ray + i]).tolist() == bits(o).tolist(), (k, i)
    img, _, lin = osc.render_rows(mode=orc.MODE_BVH, want_lin=True)
    assert np.array_equal(bits(s["shade"]["linear"]).reshape(osc.height, osc.width, 3), bits(lin))
    assert np.array_equal(s["shade"]["rgb8"].reshape(osc.height, osc.width, 3), img)


def test_helper_is_render_pixel_on_the_camera_set(orc, bunny, samples_seeded):
    s = bunny["camera"]
    assert len(s["shade"]) == W * H == 1024
    assert not np.allclose(np.linalg.norm(s["directions"], axis=1), 1.0, atol=0.5)       # the library normalises, not the caller
    check_against_render_rows(orc, bunny["osc"], s, s["px"], s["py"], 1, samples_seeded, s["cam"], orc.DISTANCE, orc.EYE)


def test_helper_is_render_pixel_with_spheres_and_two_rays(orc, soup, samples_seeded):
    """the soup through its own camera at nb_ray = 2: sphere normals, the second ray's light points, the sum across rays"""
    view = qs.SOUP_VIEW
    o, d, cam, px, py = ss.camera_raw_rays(orc, W, H, view["eye"], view["look_at"], view["up"], view["distance"],
                                           samples_seeded, nb_ray=2)
    s = ss.shade_set(orc, soup["osc2"], o, d, 2, view["nb_light_sample"], view["light_tri"], samples_seeded, soup["tables"])
    hit = s["hit"]["prim"] != NO_HIT
    assert qs.is_sphere(soup["a"], s["hit"]).sum() >= 100 and (hit & ~qs.is_sphere(soup["a"], s["hit"])).sum() >= 100
    assert (s["shade"]["hits"] == 1).sum() >= 5
    check_against_render_rows(orc, soup["osc2"], s, px, py, 2, samples_seeded, cam, view["distance"], view["eye"])


# ---------------------------------------------------------------------------------------------- conditions on the sets
def test_the_bunny_sets_hold_every_class_of_pixel(bunny):
    assert len(bunny["random"]["shade"]) == 256 and len(bunny["penumbra"]["shade"]) == ss.PENUMBRA_POINTS == 128
    c = np.concatenate([ss.classes(bunny[k]) for k in ("camera", "random", "penumbra")])
    counts = np.bincount(c, minlength=4)
    assert (counts >= 20).all(), counts       # all rays miss / every sample lit / every sample occluded / some of each
    # the line starts on lit ground, ends in the umbra, and crosses the penumbra between
    p = bunny["penumbra"]
    assert (p["hit"]["prim"] != NO_HIT).all() and p["lit"][0] == 100 and p["lit"][-1] == 0
    assert (ss.classes(p) == 3).sum() >= 20


def test_the_soup_sets_hit_spheres_and_triangles_and_half_hit_pixels(soup):
    for nb in (1, 2):
        s = soup[nb]
        assert len(s["origins"]) == 192 and len(s["shade"]) == 192 // nb
        sphere = qs.is_sphere(soup["a"], s["hit"])
        hit = s["hit"]["prim"] != NO_HIT
        assert sphere.sum() >= 10 and (hit & ~sphere).sum() >= 10
    assert (soup[2]["shade"]["hits"] == 1).sum() >= 5 and (soup[2]["shade"]["hits"] == 2).sum() >= 5
    # the same rays, the same closest hits; another pixel structure and other light points for the odd rays
    assert soup[1]["hit"].tobytes() == soup[2]["hit"].tobytes()
    assert np.isfinite(soup[1]["shade"]["linear"]).all() and np.isfinite(soup[2]["shade"]["linear"]).all()


def test_the_hard_ray_is_answered_differently_from_its_twin(bunny):
    s, twin = bunny["hard"], bunny["hard_twin"]
    assert len(s["shade"]) == 64 and np.signbit(s["directions"][63, 0]) and s["directions"][63, 0] == 0
    assert s["hit"]["prim"][63] == NO_HIT and s["shade"]["hits"][63] == 0 and not s["shade"]["linear"][63].any()
    assert twin["hit"]["prim"][0] == qs.HARD_TWIN_HITS["x"] and twin["shade"]["hits"][0] == 1
    assert twin["shade"]["linear"][0].any()
    assert s["shade"][:63].tobytes() == bunny["random"]["shade"][:63].tobytes()


def test_the_far_origin_lies_beyond_the_scene_and_hits_it(bunny):
    s = bunny["far"]
    assert len(s["shade"]) == 64 and np.abs(s["origins"][63]).max() > 100 * 1e4 / 2 and np.abs(s["origins"][:63]).max() < 1e4
    assert s["hit"]["prim"][63] != NO_HIT and np.isfinite(s["hit"]["t"][63])


# ---------------------------------------------------------------------------------------------- header, layout, exports
def header():
    return open(os.path.join(ROOT, "include", "rtx.h")).read()


def test_header_declares_the_functions_and_the_library_exports_them(rtx):
    hdr = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)
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


def test_pixel_shade_layout_in_c_ctypes_numpy_and_rust(rtx, tmp_path):
    src = tmp_path / "shade.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "rtx.h"\nint main(void) {\n'
                   'printf("%zu %zu %zu %zu %zu\\n", sizeof(RtxPixelShade), _Alignof(RtxPixelShade),\n'
                   '       offsetof(RtxPixelShade, linear), offsetof(RtxPixelShade, rgb8), offsetof(RtxPixelShade, hits));\n'
                   'return 0; }\n')
    exe = tmp_path / "shade"
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    assert subprocess.check_output([str(exe)], text=True).split() == ["16", "4", "0", "12", "15"]
    P = rtx.rtx.PixelShade
    assert C.sizeof(P) == 16 and C.alignment(P) == 4
    assert [(n, getattr(P, n).offset, getattr(P, n).size) for n, _ in P._fields_] == \
        [("linear", 0, 12), ("rgb8", 12, 3), ("hits", 15, 1)]
    dt = rtx.rtx.PIXEL_SHADE_DTYPE
    assert dt.itemsize == 16 and [(n, dt.fields[n][1]) for n in dt.names] == [("linear", 0), ("rgb8", 12), ("hits", 15)]
    assert dt == ss.SHADE_DTYPE
    rs = open(os.path.join(ROOT, "integration", "rtx_ffi.rs")).read()
    m = re.search(r"#\[repr\(C\)\]\s*(?:#\[derive\([^\)]*\)\]\s*)?pub struct RtxPixelShade \{(.*?)\n\}", rs, re.S)
    assert m, "RtxPixelShade with #[repr(C)] not found in rtx_ffi.rs"
    assert re.findall(r"pub (\w+): ([^,\n]+),", m.group(1)) == [("linear", "[f32; 3]"), ("rgb8", "[u8; 3]"), ("hits", "u8")]


def test_bad_arguments_and_empty_batches_need_no_device(rtx, scene, samples_half):
    L = rtx.rtx._lib
    f32p = rtx.rtx.f32p
    o = np.zeros((4, 3), np.float32)
    d = np.ones((4, 3), np.float32)
    shade = np.zeros(4, rtx.rtx.PIXEL_SHADE_DTYPE)
    hits = np.zeros(4, rtx.rtx.RAY_HIT_DTYPE)
    op, dp = o.ctypes.data_as(f32p), d.ctypes.data_as(f32p)
    sp, hp = shade.ctypes.data_as(C.POINTER(rtx.rtx.PixelShade)), hits.ctypes.data_as(C.POINTER(rtx.rtx.RayHit))
    h = scene.handle
    BAD, OK = rtx.ERR_BAD_ARG, rtx.OK
    # NULL pointers (out_hits may be NULL: not an error)
    assert L.rtx_shade_rays(None, 0, 4, op, dp, 0, sp, hp, None) == BAD
    assert L.rtx_shade_rays(h, 0, 4, None, dp, 0, sp, hp, None) == BAD
    assert L.rtx_shade_rays(h, 0, 4, op, None, 0, sp, hp, None) == BAD
    assert L.rtx_shade_rays(h, 0, 4, op, dp, 0, None, hp, None) == BAD
    assert L.rtx_shade_rays_device(None, 0, 4, 256, 512, 0, 768, None, None) == BAD
    assert L.rtx_shade_rays_device(h, 0, 4, None, 512, 0, 768, None, None) == BAD
    assert L.rtx_shade_rays_device(h, 0, 4, 256, None, 0, 768, None, None) == BAD
    assert L.rtx_shade_rays_device(h, 0, 4, 256, 512, 0, None, 1024, None) == BAD
    # unknown flags, more than 2^28 rays, misaligned device pointers
    assert L.rtx_shade_rays(h, 0, 4, op, dp, 4, sp, hp, None) == BAD
    assert L.rtx_shade_rays_device(h, 0, 4, 256, 512, 8, 768, None, None) == BAD
    assert L.rtx_shade_rays(h, 0, (1 << 28) + 1, op, dp, 0, sp, None, None) == BAD
    assert L.rtx_shade_rays_device(h, 0, (1 << 28) + 1, 256, 512, 0, 768, None, None) == BAD
    assert L.rtx_shade_rays_device(h, 0, 4, 256, 512, 0, 776, None, None) == BAD       # d_shade: 16-byte aligned
    assert L.rtx_shade_rays_device(h, 0, 4, 256, 512, 0, 768, 1032, None) == BAD       # d_hits too
    assert L.rtx_shade_rays_device(h, 0, 4, 258, 512, 0, 768, None, None) == BAD
    # the limit counts rays: with two rays per pixel it is 2^27 pixels
    tris, rgb = scene.tris, scene.rgb
    with rtx.Scene(16, 16, tris, rgb, samples_half[:64], tie_rank=None, nb_ray=2) as two:
        assert two.nb_ray == 2
        assert L.rtx_shade_rays(two.handle, 0, (1 << 27) + 1, op, dp, 0, sp, None, None) == BAD
        assert L.rtx_shade_rays_device(two.handle, 0, (1 << 27) + 1, 256, 512, 0, 768, None, None) == BAD
        assert L.rtx_shade_rays_device(two.handle, 0, 0, 256, 512, 0, 768, None, None) == OK
        with pytest.raises(ValueError):
            two.shade_rays(o[:3], d[:3])                   # a pixel is two rays
    # an empty batch is fine and writes nothing — also with no device at all, and whatever the flags
    shade["hits"] = 7
    hits["prim"] = 7
    st = rtx.rtx.Stats()
    st.primary_rays = 5
    assert L.rtx_shade_rays(h, 0, 0, op, dp, 0, sp, hp, None) == OK
    assert L.rtx_shade_rays(h, 0, 0, op, dp, rtx.rtx.RAYS_KEEP_ORDER, sp, None, C.byref(st)) == OK
    assert st.primary_rays == 0 and st.rays == 0 and st.primary_hits == 0 and st.shadow_rays == 0
    assert L.rtx_shade_rays_device(h, 0, 0, 256, 512, 0, 768, None, None) == OK
    assert (shade["hits"] == 7).all() and (hits["prim"] == 7).all()
    assert len(scene.shade_rays(np.zeros((0, 3)), np.zeros((0, 3)))) == 0
    with pytest.raises(ValueError):
        scene.shade_rays(o, d[:2])


def test_no_device_means_error_not_fallback(rtx, scene):
    if rtx.device_count() > 0:
        pytest.skip("a GPU is present")
    o = np.zeros((4, 3), np.float32)
    d = np.ones((4, 3), np.float32)
    for call in (lambda: scene.shade_rays(o, d), lambda: scene.shade_rays(o, d, keep_order=True, want_hits=True),
                 lambda: scene.shade_rays_device(0, 4, 256, 512, 768)):
        with pytest.raises(rtx.RtxError) as e:
            call()
        assert e.value.code == rtx.ERR_NO_DEVICE


def test_shade_kernels_live_in_their_own_namespace():
    """librtx.so carries rtxs::shade_kernel in exactly the four COUNT x SPHERES forms — the regrouping pass is the ray
    queries' (rtxq::key_kernel and the one radix sort) — and imports no getenv"""
    lib = os.path.join(ROOT, "ray-tracer-rust_amd", "librtx.so")
    blob = open(lib, "rb").read()
    shade = set(m.decode() for m in re.findall(rb"_ZN4rtxs\d+([a-z0-9_]+_kernel(?:ILb[01]ELb[01]E)?)", blob)
                if not m.startswith(b"__device_stub__"))
    forms = ["ILb%dELb%dE" % (c, s) for c in (0, 1) for s in (0, 1)]
    assert shade == {"shade_kernel" + f for f in forms}, shade
    undefined = subprocess.run(["nm", "-D", "--undefined-only", lib], capture_output=True, text=True, check=True).stdout
    assert "getenv" not in undefined


def test_the_radix_sort_is_in_the_library_once():
    """every rocprim kernel's descriptor name occurs in librtx.so as often as rtxq::key_kernel's own does: the code object
    that holds the key kernel holds the sort, and no other does"""
    blob = open(os.path.join(ROOT, "ray-tracer-rust_amd", "librtx.so"), "rb").read()
    key = re.findall(rb"_ZN4rtxq10key_kernel\w*\.kd\0", blob)
    assert len(set(key)) == 1 and len(key) >= 1, key
    counts = {}
    for name in re.findall(rb"_ZN7rocprim\w*\.kd\0", blob):
        counts[name] = counts.get(name, 0) + 1
    assert len(counts) >= 10, len(counts)                                # the sort is there at all
    more = {n[:60]: c for n, c in counts.items() if c != len(key)}
    assert not more, "%d of %d rocprim kernels occur another number of times than key_kernel's %d: %s" % (
        len(more), len(counts), len(key), sorted(more.items())[:3])
