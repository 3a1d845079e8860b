"""GPU parity of the mean of N frames: the accumulator kernels (rtx_accum_add_device, rtx_accum_resolve_device) against the
host statements word for word, and rtx_render_view_mean in both variants against the expected records of
tests/accum_sets.py — the oracle scene created with each frame's table, a float32 sum in frame order, one division,
Color::to_rgba — whose conditions tests/test_accum_sets.py asserts without a GPU.  Every comparison is for equal bits or
bytes (a NaN the statement makes stands for any NaN: the host's and the device's default NaN need not be the same word)."""
import importlib

import numpy as np
import pytest

import accum_sets as ac
import light_sets as ls
import prims_sets as pm
import resample_sets as rs
import shade_sets as ss
import view_sets as vs
from query_sets import F, bits

pytestmark = pytest.mark.gpu
GUARD = 16
BLOCK_SIZES = (1, 3, 4, 5, 63, 64, 65, 255, 256, 257, 1031)
FRAME_COUNTS = (1, 3, 7, 65536)


@pytest.fixture(scope="module")
def rtx():
    mod = importlib.import_module("ray-tracer-rust_amd")
    assert mod.device_count() >= 1, "no HIP device: the product path has no CPU fallback"
    return mod


@pytest.fixture(scope="module")
def torch():
    return pytest.importorskip("torch")


@pytest.fixture(scope="module")
def bunny(rtx, orc):
    with ac.open_bunny(rtx, ac.table(orc, 0)) as scene:
        yield scene


class Guarded:
    """`nbytes` device bytes at byte offset `offset` of an allocation filled with 0xAA, GUARD more behind them"""
    def __init__(self, torch, nbytes, offset=0):
        self.torch, self.nbytes, self.offset = torch, nbytes, offset
        self.buf = torch.full((offset + nbytes + GUARD,), 0xAA, dtype=torch.uint8, device="cuda:0")
        self.ptr = self.buf.data_ptr() + offset
        assert self.buf.data_ptr() % 16 == 0

    def put(self, array):
        raw = np.ascontiguousarray(array).view(np.uint8).reshape(-1)
        assert len(raw) == self.nbytes
        self.buf[self.offset:self.offset + self.nbytes] = self.torch.from_numpy(raw.copy()).to("cuda:0")
        return self

    def get(self, dtype=np.uint8):
        """the bytes, after the guards before and behind them were found intact"""
        self.torch.cuda.synchronize()
        raw = self.buf.cpu().numpy()
        assert (raw[:self.offset] == 0xAA).all() and (raw[self.offset + self.nbytes:] == 0xAA).all(), "guard bytes overwritten"
        return raw[self.offset:self.offset + self.nbytes].copy().view(dtype)


def stream_of(torch):
    return torch.cuda.current_stream().cuda_stream


def host_resolve(rtx, thr, acc, n_frames):
    rgb, shade = rtx.accum_resolve(thr, acc, n_frames)
    return rgb, shade


# ---------------------------------------------------------------------------------------------- 1: the building blocks
@pytest.mark.parametrize("n", BLOCK_SIZES)
def test_the_kernels_are_the_host_statements(rtx, torch, bunny, n):
    thr = bunny.gamma_thresholds()
    syn = [rec[:n] for rec in ac.synthetic(rtx)]
    d_acc = Guarded(torch, 16 * n)                                       # first over garbage: 0xAA bytes
    want = None
    for k, rec in enumerate(syn):
        d_rec = Guarded(torch, 16 * n).put(rec)
        bunny.accum_add_device(0, n, d_rec.ptr, d_acc.ptr, k == 0, stream_of(torch))
        want = rtx.accum_add(rec, want)
        got = d_acc.get(rtx.ACCUM_PIXEL_DTYPE)
        assert ac.same_accum(got, want["sum"], want["hit_frames"]), (n, k)
        assert d_rec.get(rtx.PIXEL_SHADE_DTYPE).tobytes() == rec.tobytes()                      # an add reads its records only
        if k == 0:
            assert np.array_equal(bits(got["sum"]), bits(rec["linear"])), n   # bit for bit, a NaN's payload included
    for offset, n_frames in enumerate(FRAME_COUNTS):                     # d_rgb at byte offsets 0, 1, 2, 3
        w_rgb, w_shade = host_resolve(rtx, thr, want, n_frames)
        for with_rgb, with_shade in ((True, False), (False, True), (True, True)):
            d_rgb = Guarded(torch, 3 * n, offset) if with_rgb else None
            d_shade = Guarded(torch, 16 * n) if with_shade else None
            bunny.accum_resolve_device(0, n, d_acc.ptr, n_frames, d_rgb.ptr if with_rgb else None,
                                       d_shade.ptr if with_shade else None, stream_of(torch))
            what = (n, n_frames, offset, with_rgb, with_shade)
            if with_rgb:
                assert np.array_equal(d_rgb.get().reshape(n, 3), w_rgb), what
            if with_shade:
                assert ac.same_records(d_shade.get(rtx.PIXEL_SHADE_DTYPE), w_shade), what
    assert ac.same_accum(d_acc.get(rtx.ACCUM_PIXEL_DTYPE), want["sum"], want["hit_frames"])     # a resolve reads its accumulator only
    # every offset with the frame count the statement is for
    w_rgb, _ = host_resolve(rtx, thr, want, len(syn))
    for offset in range(4):
        d_rgb = Guarded(torch, 3 * n, offset)
        bunny.accum_resolve_device(0, n, d_acc.ptr, len(syn), d_rgb.ptr, None, stream_of(torch))
        assert np.array_equal(d_rgb.get().reshape(n, 3), w_rgb), (n, offset)


def test_three_hundred_adds_pin_hits_at_255(rtx, torch, bunny):
    thr = bunny.gamma_thresholds()
    n = 5
    rec = np.zeros(n, rtx.PIXEL_SHADE_DTYPE)
    rec["linear"] = np.array([[0.001, 0.25, 1.0 / 3.0], [1e-40, 0.0, -0.0], [0.1, 0.2, 0.3], [2.0 ** -61, 1.0, 0.7], [0.0, 0.0, 0.0]], F)
    rec["hits"] = [1, 255, 2, 0, 1]
    d_rec, d_acc, d_shade = Guarded(torch, 16 * n).put(rec), Guarded(torch, 16 * n), Guarded(torch, 16 * n)
    want = None
    for k in range(300):
        bunny.accum_add_device(0, n, d_rec.ptr, d_acc.ptr, k == 0, stream_of(torch))
        want = rtx.accum_add(rec, want)
    got = d_acc.get(rtx.ACCUM_PIXEL_DTYPE)
    assert got["hit_frames"].tolist() == [300, 300, 300, 0, 300] and ac.same_accum(got, want["sum"], want["hit_frames"])
    bunny.accum_resolve_device(0, n, d_acc.ptr, 300, None, d_shade.ptr, stream_of(torch))
    shade = d_shade.get(rtx.PIXEL_SHADE_DTYPE)
    assert shade["hits"].tolist() == [255, 255, 255, 0, 255]
    assert ac.same_records(shade, host_resolve(rtx, thr, want, 300)[1])


def test_records_of_a_view_call_and_of_a_shade_call(rtx, torch, orc, bunny):
    """an add takes the records of ANY call that writes RtxPixelShade: rtx_render_view_device's and rtx_shade_rays_device's
    for the same rays, two frames of each, against the host statements over the host calls' records"""
    thr = bunny.gamma_thresholds()
    view = bunny.own_view()
    w, h = ac.BUNNY_FRAME
    n = w * h
    o, d, _, _, _ = ss.camera_raw_rays(orc, w, h, rtx.DEFAULT_EYE, rtx.DEFAULT_LOOK_AT, rtx.DEFAULT_UP, rtx.DEFAULT_DISTANCE,
                                       ac.table(orc, 0), 1)
    d_o, d_d = (torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0") for a in (o, d))
    _, host_view = bunny.render_view(view, want_shade=True)
    host_shade = bunny.shade_rays(o, d)
    assert host_view.reshape(-1).tobytes() == host_shade.tobytes() and (host_shade["hits"] != 0).sum() > 500
    d_rec, d_acc, d_out = Guarded(torch, 16 * n), Guarded(torch, 16 * n), Guarded(torch, 16 * n)
    d_rgb = Guarded(torch, 3 * n, 3)
    stream = stream_of(torch)
    bunny.render_view_device(0, view, d_shade_ptr=d_rec.ptr, stream=stream)
    bunny.accum_add_device(0, n, d_rec.ptr, d_acc.ptr, True, stream)
    bunny.shade_rays_device(0, n, d_o.data_ptr(), d_d.data_ptr(), d_rec.ptr, stream=stream)
    bunny.accum_add_device(0, n, d_rec.ptr, d_acc.ptr, False, stream)
    bunny.accum_resolve_device(0, n, d_acc.ptr, 2, d_rgb.ptr, d_out.ptr, stream)
    want = rtx.accum_add(host_shade, rtx.accum_add(host_shade))
    w_rgb, w_shade = host_resolve(rtx, thr, want, 2)
    assert ac.same_accum(d_acc.get(rtx.ACCUM_PIXEL_DTYPE), want["sum"], want["hit_frames"])
    assert ac.same_records(d_out.get(rtx.PIXEL_SHADE_DTYPE), w_shade) and np.array_equal(d_rgb.get().reshape(n, 3), w_rgb)
    assert np.array_equal(w_rgb.reshape(h, w, 3), bunny.render_view(view))              # the mean of a frame with itself


# ---------------------------------------------------------------------------------------------- 2: the mean call
def check_mean(rtx, got_rgb, got_shade, e, what):
    assert np.array_equal(bits(got_shade["linear"]), bits(e["linear"])), "%s: %d pixels' linear words differ" % (
        what, (bits(got_shade["linear"]) != bits(e["linear"])).any(axis=-1).sum())
    assert np.array_equal(got_shade["rgb8"], e["rgb8"]), "%s: %d pixels' bytes differ" % (what, (got_shade["rgb8"] != e["rgb8"]).any(axis=-1).sum())
    assert np.array_equal(got_shade["hits"], e["hits"]), what + ": hits differ"
    if got_rgb is not None:
        assert np.array_equal(got_rgb, e["rgb8"]), what + ": out_rgb is not the records' bytes"


def mean_on_device(rtx, torch, scene, view, seeds, n_pairs, rgb_offset=1, **kw):
    """rtx_render_view_mean_device into guarded buffers -> (rgb, shade, accum)"""
    h, w = view.ny, view.nx
    d_acc, d_shade, d_rgb = Guarded(torch, 16 * w * h), Guarded(torch, 16 * w * h), Guarded(torch, 3 * w * h, rgb_offset)
    scene.render_view_mean_device(0, view, seeds, n_pairs, d_acc.ptr, d_rgb.ptr, d_shade.ptr, stream_of(torch), **kw)
    return (d_rgb.get().reshape(h, w, 3), d_shade.get(rtx.PIXEL_SHADE_DTYPE).reshape(h, w), d_acc.get(rtx.ACCUM_PIXEL_DTYPE).reshape(h, w))


@pytest.mark.parametrize("n", ac.FRAME_COUNTS)
def test_the_bunnys_mean_is_the_expected_record(rtx, torch, orc, bunny, n):
    e = ac.expected(orc, rtx, "bunny", n)
    view = bunny.own_view()
    rgb, shade, st = bunny.render_view_mean(view, ac.SEEDS[:n], ac.N_PAIRS, want_shade=True, stats=True)
    check_mean(rtx, rgb, shade, e, "host variant, %d frames" % n)
    w, h = ac.BUNNY_FRAME
    hits = sum(int(f["hit"].sum()) for f in ac.frames(orc, rtx, "bunny", n))
    assert st["primary_rays"] == n * w * h and st["primary_hits"] == hits and st["shadow_rays"] == hits * ac.BUNNY_LIGHT_SAMPLES
    assert st["kernel_ms"] > 0
    assert np.array_equal(bunny.render_view_mean(view, ac.SEEDS[:n], ac.N_PAIRS), e["rgb8"])       # rgb alone, uncounted
    d_rgb, d_shade, d_acc = mean_on_device(rtx, torch, bunny, view, ac.SEEDS[:n], ac.N_PAIRS)
    check_mean(rtx, d_rgb, d_shade, e, "device variant, %d frames" % n)
    assert ac.same_accum(d_acc, e["sum"], e["hit_frames"])


def test_the_yards_mean_unposed_and_posed(rtx, torch, orc):
    view = ac.yard_view(rtx)
    with rs.open_yard(rtx, ac.table(orc, 3)) as scene:
        with pytest.raises(rtx.RtxError) as refused:                     # a posed mean on a device without a pose
            scene.render_view_mean(view, ac.SEEDS[:3], ac.N_PAIRS, posed=True)
        assert refused.value.code == rtx.ERR_BAD_ARG
        scene.pose_prims(**pm.given(rtx, ac.YARD_POSE[1]))
        for fixture, posed in (("yard", False), ("yard_posed", True), ("yard", False)):
            e = ac.expected(orc, rtx, fixture, ac.YARD_FRAMES)
            rgb, shade, st = scene.render_view_mean(view, ac.SEEDS[:3], ac.N_PAIRS, posed=posed, want_shade=True, stats=True)
            check_mean(rtx, rgb, shade, e, fixture + ", host variant")
            assert st["primary_rays"] == 3 * view.nx * view.ny * pm.NB_RAY
            d_rgb, d_shade, d_acc = mean_on_device(rtx, torch, scene, view, ac.SEEDS[:3], ac.N_PAIRS, rgb_offset=2, posed=posed)
            check_mean(rtx, d_rgb, d_shade, e, fixture + ", device variant")
            assert ac.same_accum(d_acc, e["sum"], e["hit_frames"])


def lit_expected(orc, rtx, light, n, rect=None):
    """accum_sets' statement over the bunny under `light`, frames 0 .. n-1"""
    acc = None
    for k in range(n):
        osc = orc.default_scene(["bunny.obj"], ac.BUNNY_FRAME[0], ac.BUNNY_FRAME[1], ac.table(orc, k), light_tri=light[0],
                                nb_light_sample=light[1])
        _, _, tri, lin = osc.render_rows(mode=orc.MODE_BVH, want_tri=True, want_lin=True)
        osc.close()
        acc = ac.np_add(lin, tri != 0xFFFFFFFF, acc)
    linear = ac.np_divide(acc[0], n)
    return dict(linear=linear, rgb8=ac.oracle_bytes(orc, linear), hits=np.minimum(acc[1], 255).astype(np.uint8), sum=acc[0], hit_frames=acc[1])


def test_another_light_with_a_count_of_seven(rtx, torch, orc, bunny):
    tri, count = ls.SIDE_LIGHTS["far_side"][0], 7
    e = lit_expected(orc, rtx, (tri, count), 3)
    assert (e["rgb8"] != ac.expected(orc, rtx, "bunny", 3)["rgb8"]).any()
    light = rtx.Scene.make_light(tri, count)
    view = bunny.own_view()
    rgb, shade, st = bunny.render_view_mean(view, ac.SEEDS[:3], ac.N_PAIRS, light=light, want_shade=True, stats=True)
    check_mean(rtx, rgb, shade, e, "far_side x 7, host variant")
    assert st["shadow_rays"] == 7 * st["primary_hits"]
    d_rgb, d_shade, _ = mean_on_device(rtx, torch, bunny, view, ac.SEEDS[:3], ac.N_PAIRS, light=light)
    check_mean(rtx, d_rgb, d_shade, e, "far_side x 7, device variant")
    # a count of 0 is the scene's count; no light is the scene's light: the unlit fixture again
    own = bunny.light()
    own.nb_light_sample = 0
    check_mean(rtx, *bunny.render_view_mean(view, ac.SEEDS[:3], ac.N_PAIRS, light=own, want_shade=True), ac.expected(orc, rtx, "bunny", 3),
               "the scene's own light, given")


def test_a_rectangle_off_the_tile_grid(rtx, torch, orc):
    """x0 = 3, y0 = 5, 13 x 9 of the yard's view: the rectangle holds the horizon, pixels hit in every frame, in some and in none"""
    x0, y0, nx, ny = 3, 5, 13, 9
    (w, h), eye, look_at, distance = ac.YARD_MEAN_VIEW
    view = rtx.Scene.view(w, h, eye, look_at, vs.UP, distance, rect=(x0, y0, nx, ny))
    whole = ac.expected(orc, rtx, "yard", ac.YARD_FRAMES)
    e = {k: whole[k][y0:y0 + ny, x0:x0 + nx] for k in whole}
    assert (e["hits"] == 3).any() and (e["hits"] == 0).any() and ((e["hits"] > 0) & (e["hits"] < 3)).any()
    seeds = ac.SEEDS[:ac.YARD_FRAMES]
    with rs.open_yard(rtx, ac.table(orc, 5)) as scene:
        rgb, shade = scene.render_view_mean(view, seeds, ac.N_PAIRS, want_shade=True)
        check_mean(rtx, rgb, shade, e, "rectangle, host variant")
        for offset in range(4):
            d_rgb, d_shade, d_acc = mean_on_device(rtx, torch, scene, view, seeds, ac.N_PAIRS, rgb_offset=offset)
            check_mean(rtx, d_rgb, d_shade, e, "rectangle, device variant, offset %d" % offset)
            assert ac.same_accum(d_acc, e["sum"], e["hit_frames"])


def test_tables_shorter_and_longer_than_the_scenes_own(rtx, torch, orc):
    """the scratch table is reused and grown: n_pairs below and above the scene's own table size, in both orders, against a
    twin scene reseeded to each frame's table (rtx_render_view_lit's records through the host statements)"""
    own = ac.table(orc, 0)[:1000]
    thr = None
    for order in ((7, 5003, 129, 6007), (6007, 129, 5003, 7)):
        with ac.open_bunny(rtx, own) as scene, ac.open_bunny(rtx, own) as twin:
            thr = scene.gamma_thresholds()
            view = scene.own_view()
            light = scene.light()
            for n_pairs in order:
                seeds = (11, 2 ** 64 - 1, 12)
                acc = None
                for seed in seeds:
                    twin.reseed(seed, n_pairs)
                    acc = rtx.accum_add(twin.render_view(view, want_shade=True, light=light)[1], acc)
                w_rgb, w_shade = rtx.accum_resolve(thr, acc, len(seeds))
                rgb, shade = scene.render_view_mean(view, seeds, n_pairs, want_shade=True)
                assert shade.tobytes() == w_shade.tobytes() and np.array_equal(rgb, w_rgb), (order, n_pairs)
                d_rgb, d_shade, _ = mean_on_device(rtx, torch, scene, view, seeds, n_pairs)
                assert d_shade.tobytes() == w_shade.tobytes() and np.array_equal(d_rgb, w_rgb), (order, n_pairs)
            # one frame is that frame's record, hits clipped to 0 or 1
            twin.reseed(5, 4099)
            _, one = twin.render_view(view, want_shade=True, light=light)
            _, shade = scene.render_view_mean(view, (5,), 4099, want_shade=True)
            assert np.array_equal(bits(shade["linear"]), bits(one["linear"])) and np.array_equal(shade["rgb8"], one["rgb8"])
            assert np.array_equal(shade["hits"], np.minimum(one["hits"], 1))


# ---------------------------------------------------------------------------------------------- 3: state
def test_a_mean_call_leaves_the_scene_untouched(rtx, torch, orc):
    with rs.open_yard(rtx, ac.table(orc, 4)) as scene, rs.open_yard(rtx, ac.table(orc, 4)) as fresh:
        view = scene.own_view()

        def state():
            return (scene.debug_samples().tobytes(), scene.samples_at().tobytes(), scene.render_rows().tobytes(),
                    scene.render_view_rows(view).tobytes(), scene.render_view(view, want_shade=True)[1].tobytes(),
                    scene.debug_light_points(scene.light()).tobytes(), scene.info())

        before = state()
        scene.render_view_mean(ac.yard_view(rtx), ac.SEEDS[:3], ac.N_PAIRS)
        mean_on_device(rtx, torch, scene, ac.yard_view(rtx), ac.SEEDS[:3], 7001, light=rtx.Scene.make_light(*pm.POSE_LIGHT))
        assert state() == before
        # a reseed + render after a mean call is a fresh scene's
        scene.reseed(77, 5003)
        fresh.reseed(77, 5003)
        assert scene.render_rows().tobytes() == fresh.render_rows().tobytes()
        assert scene.render_view(view, want_shade=True)[1].tobytes() == fresh.render_view(view, want_shade=True)[1].tobytes()
        assert scene.debug_samples().tobytes() == fresh.debug_samples().tobytes()


def test_two_device_resident_means_on_a_stream_of_their_own_and_a_host_mean_behind_them(rtx, torch, orc, bunny):
    """device-resident launches on one device are ordered on one stream; the host entry point waits for the most recent of
    them by an event before it reuses the scratch table, the scratch records and the light points"""
    view = bunny.own_view()
    w, h = ac.BUNNY_FRAME
    e7, e3, e8 = (ac.expected(orc, rtx, "bunny", n) for n in (7, 3, 8))
    side = torch.cuda.Stream()
    bufs = [(Guarded(torch, 16 * w * h), Guarded(torch, 16 * w * h), Guarded(torch, 3 * w * h, 1)) for _ in range(2)]
    torch.cuda.synchronize()                                             # (the buffers were filled on torch's own stream)
    for (d_acc, d_shade, d_rgb), n in zip(bufs, (7, 3)):
        bunny.render_view_mean_device(0, view, ac.SEEDS[:n], ac.N_PAIRS, d_acc.ptr, d_rgb.ptr, d_shade.ptr, side.cuda_stream)
    rgb, shade = bunny.render_view_mean(view, ac.SEEDS[:8], ac.N_PAIRS, want_shade=True)          # nothing waited for in between
    side.synchronize()
    check_mean(rtx, rgb, shade, e8, "host variant behind two device-resident calls")
    for (d_acc, d_shade, d_rgb), e in zip(bufs, (e7, e3)):
        check_mean(rtx, d_rgb.get().reshape(h, w, 3), d_shade.get(rtx.PIXEL_SHADE_DTYPE).reshape(h, w), e, "device-resident, side stream")
        assert ac.same_accum(d_acc.get(rtx.ACCUM_PIXEL_DTYPE).reshape(h, w), e["sum"], e["hit_frames"])
