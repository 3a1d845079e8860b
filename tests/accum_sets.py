"""Fixtures for the tests of the mean of N frames (rtx_render_view_mean, rtx_accum_add_device, rtx_accum_resolve_device,
rtxh_accum_add, rtxh_accum_resolve), with the CPU oracle's answers: numpy, the oracle binding and the library's host side
only, no GPU.

The expected record of pixel p over n frames is stated here once, in numpy: frame k is the ORACLE SCENE CREATED WITH THE TABLE
gen_samples(SEEDS[k], N_PAIRS), rendered whole (render_rows: linear colour and first ray's primitive per pixel); the linear
colours are added in frame order in float32 starting from frame 0's own words, the sum is divided once by float32(n), and the
bytes are orc_color_to_rgb8 of that quotient; hits is the number of frames in which the pixel had a closest hit.

Three fixtures:
    bunny        bunny.obj + ground, 48 x 32, main()'s camera and light, one ray per pixel, 10 light samples, at FRAME_COUNTS
    yard         resample_sets' yard — 41 triangles, 5 spheres, two rays per pixel, ten light samples, 24 x 16 — at 3 frames,
                 seen through YARD_MEAN_VIEW: from the yard's own camera every pixel below the horizon is hit in every frame and
                 none above it in any (the horizon lies on a row boundary), so no pixel would be hit in some frames only; from
                 this low eye the spheres and the mesh stand against the sky.  The library's scene keeps its own camera: the
                 mean call is handed the view
    yard_posed   the same under prims_sets' pose "all"
and SYNTHETIC_N synthetic records per frame that hold what no render produces: -0.0, denormals, 2^61 and 2^-61, infinities of
both signs, NaN, and hits of 0, 1 and 255.
tests/test_accum_sets.py asserts, without a GPU, that the fixtures can tell a wrong order, a reciprocal, a dropped frame or a
byte taken from one frame from the statement; tests/test_accum_host.py and tests/test_gpu_accum.py use them.  Everything is
built once per process (query_sets._once) and read-only."""
import ctypes as C
import os

import numpy as np

import prims_sets as pm
import query_sets as qs
import resample_sets as rs
import shade_sets as ss
import view_sets as vs
from query_sets import F, NO_HIT

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEEDS = (0, 1, 2 ** 64 - 1, 20261020, 5, 6, 7, 8)
N_PAIRS = 4099
FRAME_COUNTS = (1, 3, 7, 8)
BUNNY_FRAME = (48, 32)
BUNNY_LIGHT_SAMPLES = 10
YARD_FRAMES = 3
YARD_POSE = ("prims", "all")
YARD_MEAN_VIEW = ((24, 16), (0.0, 20.0, 150.0), (5.0, 24.0, 0.0), 26.0)
SYNTHETIC_N = 1031
SYNTHETIC_FRAMES = 4
MAX_FRAMES = 65536


def table(orc, k):
    return qs._once("accum_table_%d" % k, lambda: _frozen(orc.gen_samples(SEEDS[k], N_PAIRS)))


def _frozen(a):
    a.setflags(write=False)
    return a


# ---------------------------------------------------------------------------------------------- the frames
def open_bunny(binding, samples):
    """either binding's bunny scene with `samples` as its table"""
    name = "bunny.obj" if binding.__name__ == "orclib" else os.path.join(ROOT, "models", "bunny.obj")
    return binding.default_scene([name], BUNNY_FRAME[0], BUNNY_FRAME[1], samples, nb_light_sample=BUNNY_LIGHT_SAMPLES)


def bunny_frame(orc, k):
    """frame k of the bunny by the oracle: dict(lin float32 [h, w, 3], hit bool [h, w], rgb8 uint8 [h, w, 3])"""
    def make():
        osc = open_bunny(orc, table(orc, k))
        frame, _, tri, lin = osc.render_rows(mode=orc.MODE_BVH, want_tri=True, want_lin=True)
        osc.close()
        return dict(lin=_frozen(lin), hit=_frozen(tri != NO_HIT), rgb8=_frozen(frame))
    return qs._once("accum_bunny_%d" % k, make)


def yard_frame(orc, rtx, k, posed):
    """frame k of the yard (posed: under YARD_POSE).  Two rays per pixel: a pixel has a hit when either ray has one, which the
    oracle's per-pixel primitive (ray 0's) does not say, so both rays are made and asked"""
    def make():
        prims = rs.posed_prims(rtx, None, YARD_POSE) if posed else pm.yard(rtx)
        t = table(orc, k)
        osc = rs.yard_oracle(orc, prims, t, **vs.camera(YARD_MEAN_VIEW))
        frame, _, tri, lin = osc.render_rows(mode=orc.MODE_BVH, want_tri=True, want_lin=True)
        (w, h), eye, look_at, distance = YARD_MEAN_VIEW
        o, d, _, _, _ = ss.camera_raw_rays(orc, w, h, eye, look_at, vs.UP, distance, t, pm.NB_RAY)
        exp, _ = qs.oracle_hits(orc, osc, o, d, qs.HIT_DTYPE)
        osc.close()
        hit = (exp["prim"] != NO_HIT).reshape(h, w, pm.NB_RAY)
        assert np.array_equal(hit[:, :, 0], tri != NO_HIT)
        return dict(lin=_frozen(lin), hit=_frozen(hit.any(axis=2)), rgb8=_frozen(frame))
    return qs._once("accum_yard_%d_%s" % (k, posed), make)


def yard_view(rtx):
    """YARD_MEAN_VIEW as the RtxView a mean call is handed"""
    (w, h), eye, look_at, distance = YARD_MEAN_VIEW
    return rtx.Scene.view(w, h, eye, look_at, vs.UP, distance)


def frames(orc, rtx, fixture, n):
    if fixture == "bunny":
        return [bunny_frame(orc, k) for k in range(n)]
    return [yard_frame(orc, rtx, k, fixture == "yard_posed") for k in range(n)]


# ---------------------------------------------------------------------------------------------- the statement in numpy
def np_add(lin, hit, acc=None):
    """accum_add_statement over arrays: lin float32 [..., 3], hit bool [...]; acc: None (first) or (sum, hit_frames)"""
    if acc is None:
        return lin.astype(F).copy(), hit.astype(np.uint32)
    with np.errstate(invalid="ignore", over="ignore"):
        return (acc[0] + lin).astype(F), (acc[1] + hit.astype(np.uint32)).astype(np.uint32)


def np_divide(total, n):
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        return (total / F(n)).astype(F)


def np_bytes(thr, x):
    """quantise_statement over an array: the number of thresholds thr[1 .. 255] that are <= x; -inf counts as +inf, a NaN
    loses every comparison"""
    x = np.where(x == -np.inf, np.inf, x).astype(F)
    with np.errstate(invalid="ignore"):
        return (x[..., None] >= thr[1:]).sum(axis=-1).astype(np.uint8)


def oracle_bytes(orc, lin):
    out = np.zeros(lin.shape, np.uint8)
    flat_in, flat_out = np.ascontiguousarray(lin, F).reshape(-1, 3), out.reshape(-1, 3)
    buf = (C.c_uint8 * 3)()
    for i in range(len(flat_in)):
        orc.lib().orc_color_to_rgb8(orc._fp(flat_in[i]), buf)
        flat_out[i] = buf[0], buf[1], buf[2]
    return out


def ordered_sum(lins, order=None):
    """float32 sequential sum of the frames' linear colours in `order` (default: frame order), from the first one's words"""
    order = range(len(lins)) if order is None else order
    total = None
    for k in order:
        total = lins[k].astype(F).copy() if total is None else (total + lins[k]).astype(F)
    return total


def expected(orc, rtx, fixture, n):
    """dict(linear float32 [h, w, 3], rgb8 uint8 [h, w, 3], hits uint8 [h, w], sum, hit_frames) of the mean of frames 0 .. n-1"""
    def make():
        fr = frames(orc, rtx, fixture, n)
        acc = None
        for f in fr:
            acc = np_add(f["lin"], f["hit"], acc)
        linear = np_divide(acc[0], n)
        out = dict(linear=linear, rgb8=oracle_bytes(orc, linear), hits=np.minimum(acc[1], 255).astype(np.uint8), sum=acc[0],
                   hit_frames=acc[1])
        for a in out.values():
            a.setflags(write=False)
        return out
    return qs._once("accum_expected_%s_%d" % (fixture, n), make)


def as_records(rtx, linear, rgb8, hits):
    out = np.zeros(hits.shape, rtx.PIXEL_SHADE_DTYPE)
    out["linear"], out["rgb8"], out["hits"] = linear, rgb8, hits
    return out


def frame_records(rtx, frame):
    """an oracle frame as the RtxPixelShade records a view call gives for it (hits: 0 or 1 stands for any count)"""
    return as_records(rtx, frame["lin"], frame["rgb8"], frame["hit"].astype(np.uint8))


def same_records(got, want):
    """word for word, a NaN standing for any NaN"""
    gl, wl = qs.bits(got["linear"]), qs.bits(want["linear"])
    nan = np.isnan(want["linear"])
    return (np.array_equal(np.isnan(got["linear"]), nan) and np.array_equal(gl[~nan], wl[~nan])
            and np.array_equal(got["rgb8"], want["rgb8"]) and np.array_equal(got["hits"], want["hits"]))


def same_accum(got, want_sum, want_hit_frames):
    nan = np.isnan(want_sum)
    return (np.array_equal(np.isnan(got["sum"]), nan) and np.array_equal(qs.bits(got["sum"])[~nan], qs.bits(want_sum)[~nan])
            and np.array_equal(got["hit_frames"], want_hit_frames))


# ---------------------------------------------------------------------------------------------- synthetic records
SPECIALS = (-0.0, 0.0, 1e-45, -1e-45, 1e-40, 2.0 ** 61, -2.0 ** 61, 2.0 ** -61, np.inf, -np.inf, np.nan, 1.0, 0.5, 3.0e38,
            0.21404114, 1.0000001, 0.99999994)


def synthetic(rtx):
    """SYNTHETIC_FRAMES arrays of SYNTHETIC_N RtxPixelShade records: a third of the words from SPECIALS, the others uniform in
    [0, 1); hits from (0, 1, 255, 2); rgb8 arbitrary (an add does not read it).  Record 0 of every frame is a hit, record 1 of
    none, and records 2 .. 4 hold an infinity that meets its opposite in frame 1."""
    def make():
        rng = np.random.default_rng(20261021)
        out = []
        for k in range(SYNTHETIC_FRAMES):
            lin = rng.random((SYNTHETIC_N, 3)).astype(F)
            pick = rng.random((SYNTHETIC_N, 3)) < 1.0 / 3.0
            lin[pick] = np.array(SPECIALS, F)[rng.integers(0, len(SPECIALS), int(pick.sum()))]
            hits = np.array((0, 1, 255, 2), np.uint8)[rng.integers(0, 4, SYNTHETIC_N)]
            hits[0], hits[1] = 1, 0
            lin[2:5] = np.inf if k != 1 else -np.inf
            rec = as_records(rtx, lin, rng.integers(0, 256, (SYNTHETIC_N, 3)).astype(np.uint8), hits)
            out.append(_frozen(rec))
        return out
    return qs._once("accum_synthetic", make)


def synthetic_accum(rtx, n_frames=SYNTHETIC_FRAMES):
    """the numpy statement over the first n_frames synthetic frames -> (sum, hit_frames)"""
    acc = None
    for rec in synthetic(rtx)[:n_frames]:
        acc = np_add(rec["linear"], rec["hits"] != 0, acc)
    return acc


def np_resolve(rtx, thr, total, hit_frames, n):
    linear = np_divide(total, n)
    return as_records(rtx, linear, np_bytes(thr, linear), np.minimum(hit_frames, 255).astype(np.uint8))
