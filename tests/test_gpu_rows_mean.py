"""GPU parity of rtx_render_view_rows_mean (and its device-resident variant): the mean of N seeded frames through the render
pipeline against accum_sets' expected records (the oracle's frames, added in numpy) and against rtx_render_view_mean on the
same arguments — linear words, bytes, hits and the accumulator, word for word — the scene untouched afterwards, and the
three families of mean calls back to back on the scratch they share."""
import importlib

import numpy as np
import pytest

import accum_sets as ac
import light_sets as ls
import prims_sets as pm
import resample_sets as rs
from query_sets import NO_HIT, bits

pytestmark = pytest.mark.gpu
GUARD = 64


@pytest.fixture(scope="module")
def rtx():
    mod = importlib.import_module("ray-tracer-rust_amd")
    assert mod.device_count() >= 1, "no HIP device: the product path has no CPU fallback"
    return mod


@pytest.fixture(scope="module")
def torch():
    t = pytest.importorskip("torch")
    assert t.cuda.is_available(), "torch sees no GPU"
    return t


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

    def get(self, dtype=np.uint8):
        self.torch.cuda.synchronize()
        raw = self.buf.cpu().numpy()
        assert (raw[:self.offset] == 0xAA).all() and (raw[self.offset + self.nbytes:] == 0xAA).all(), "guard bytes overwritten"
        return raw[self.offset:self.offset + self.nbytes].copy().view(dtype)


def check_mean(got_rgb, got_shade, e, what):
    assert ac.same_records(got_shade, e), "%s: %d pixels' records differ" % (
        what, ((bits(got_shade["linear"]) != bits(e["linear"])).any(axis=-1) | (got_shade["hits"] != e["hits"])).sum())
    assert np.array_equal(got_rgb, e["rgb8"]), what + ": out_rgb is not the records' bytes"


def on_device(rtx, torch, scene, view, seeds, n_pairs, rows, stream=None, **kw):
    """the device-resident mean into guarded buffers -> (rgb, shade, accum)"""
    h, w = view.ny, view.nx
    d_acc, d_shade, d_rgb = Guarded(torch, 16 * w * h), Guarded(torch, 16 * w * h), Guarded(torch, 3 * w * h, 1)
    torch.cuda.synchronize()
    scene.render_view_mean_device(0, view, seeds, n_pairs, d_acc.ptr, d_rgb.ptr, d_shade.ptr,
                                  stream or torch.cuda.current_stream().cuda_stream, rows=rows, **kw)
    return (d_rgb.get().reshape(h, w, 3), d_shade.get(rtx.PIXEL_SHADE_DTYPE).reshape(h, w), d_acc.get(rtx.ACCUM_PIXEL_DTYPE).reshape(h, w))


def both_ways(rtx, torch, scene, view, seeds, n_pairs, what, e=None, **kw):
    """the rows mean, host and device-resident, against rtx_render_view_mean on the same arguments (and the expected record)"""
    v_rgb, v_shade, v_st = scene.render_view_mean(view, seeds, n_pairs, want_shade=True, stats=True, **kw)
    rgb, shade, st = scene.render_view_mean(view, seeds, n_pairs, want_shade=True, stats=True, rows=True, **kw)
    check_mean(rgb, shade, v_shade, what + ": host variant against rtx_render_view_mean")
    assert np.array_equal(rgb, v_rgb)
    for k in ("primary_rays", "primary_hits", "shadow_rays", "rays"):
        assert st[k] == v_st[k], (what, k, st[k], v_st[k])
    assert st["kernel_ms"] > 0
    assert np.array_equal(scene.render_view_mean(view, seeds, n_pairs, rows=True, **kw), rgb), what + ": rgb alone, uncounted"
    _, _, v_acc = on_device(rtx, torch, scene, view, seeds, n_pairs, False, **kw)
    d_rgb, d_shade, d_acc = on_device(rtx, torch, scene, view, seeds, n_pairs, True, **kw)
    check_mean(d_rgb, d_shade, v_shade, what + ": device variant against rtx_render_view_mean")
    assert ac.same_accum(d_acc, v_acc["sum"], v_acc["hit_frames"]), what + ": the accumulator"
    if e is not None:
        check_mean(rgb, shade, e, what + ": against the expected record")
        assert ac.same_accum(d_acc, e["sum"], e["hit_frames"])
    return shade


@pytest.mark.parametrize("n", ac.FRAME_COUNTS)
def test_the_bunnys_mean(rtx, torch, orc, bunny, n):
    e = ac.expected(orc, rtx, "bunny", n)
    shade = both_ways(rtx, torch, bunny, bunny.own_view(), ac.SEEDS[:n], ac.N_PAIRS, "bunny, %d frames" % n, e)
    if n >= 3:
        assert ((shade["hits"] > 0) & (shade["hits"] < n)).sum() >= 10          # pixels hit in some frames only


def test_the_yards_mean_unposed_and_posed(rtx, torch, orc):
    view = ac.yard_view(rtx)
    with rs.open_yard(rtx, ac.table(orc, 3)) as scene:
        with pytest.raises(rtx.RtxError) as refused:                     # a posed mean on a device without a pose
            scene.render_view_mean(view, ac.SEEDS[:3], ac.N_PAIRS, posed=True, rows=True)
        assert refused.value.code == rtx.ERR_BAD_ARG
        scene.pose_prims(**pm.given(rtx, ac.YARD_POSE[1]))
        for fixture, posed in (("yard", False), ("yard_posed", True), ("yard", False)):
            both_ways(rtx, torch, scene, view, ac.SEEDS[:3], ac.N_PAIRS, fixture, ac.expected(orc, rtx, fixture, ac.YARD_FRAMES), posed=posed)


def test_another_light_with_a_count_of_seven(rtx, torch, orc, bunny):
    light = rtx.Scene.make_light(ls.SIDE_LIGHTS["far_side"][0], 7)
    lit = both_ways(rtx, torch, bunny, bunny.own_view(), ac.SEEDS[:3], ac.N_PAIRS, "far_side x 7", light=light)
    assert (lit["rgb8"] != ac.expected(orc, rtx, "bunny", 3)["rgb8"]).any()
    own = bunny.light()
    own.nb_light_sample = 0                                              # the scene's own light, given: the unlit fixture again
    both_ways(rtx, torch, bunny, bunny.own_view(), ac.SEEDS[:3], ac.N_PAIRS, "own light, given", ac.expected(orc, rtx, "bunny", 3), light=own)


def test_tables_shorter_and_longer_than_the_scenes_own_and_row_windows(rtx, torch, orc):
    own = ac.table(orc, 0)[:1000]
    with ac.open_bunny(rtx, own) as scene:
        view = scene.own_view()
        for n_pairs in (7, 5003, 7):
            both_ways(rtx, torch, scene, view, (11, 2 ** 64 - 1, 12), n_pairs, "n_pairs %d" % n_pairs)
        w, h = ac.BUNNY_FRAME
        whole = scene.render_view_mean(view, ac.SEEDS[:3], ac.N_PAIRS, want_shade=True)[1]
        v = scene.own_view()
        v.y0, v.ny = 3, 13
        got = scene.render_view_mean(v, ac.SEEDS[:3], ac.N_PAIRS, want_shade=True, rows=True)[1]
        assert ac.same_records(got, whole[3:16]), "rows [3, 16)"
        # not the full width: refused, whatever else holds
        v.x0, v.nx = 1, w - 1
        with pytest.raises(rtx.RtxError) as e:
            scene.render_view_mean(v, ac.SEEDS[:3], ac.N_PAIRS, rows=True)
        assert e.value.code == rtx.ERR_BAD_ARG


def test_a_rows_mean_leaves_the_scene_untouched(rtx, torch, orc):
    with rs.open_yard(rtx, ac.table(orc, 4)) as scene, rs.open_yard(rtx, ac.table(orc, 4)) as fresh:
        view = scene.own_view()
        scene.pose_prims(**pm.given(rtx, "all"))

        def state():
            return (scene.debug_samples().tobytes(), scene.samples_at().tobytes(), scene.render_rows().tobytes(),
                    scene.render_view_rows(view).tobytes(), scene.render_view_rows_shade(view, posed=True).tobytes(),
                    scene.render_view(view, want_shade=True)[1].tobytes(), scene.debug_light_points(scene.light()).tobytes(),
                    scene.debug_light_walk(scene.light())[0].tobytes(), scene.debug_aimed_nodes(tuple(view.eye)).tobytes(),
                    scene.debug_pose()[0].tobytes(), scene.info())

        before = state()
        scene.render_view_mean(ac.yard_view(rtx), ac.SEEDS[:3], ac.N_PAIRS, rows=True)
        on_device(rtx, torch, scene, ac.yard_view(rtx), ac.SEEDS[:3], 7001, True, light=rtx.Scene.make_light(*pm.POSE_LIGHT), posed=True)
        assert state() == before
        scene.reseed(77, 5003)                                           # a reseed + render after a mean call is a fresh scene's
        fresh.reseed(77, 5003)
        assert scene.render_rows().tobytes() == fresh.render_rows().tobytes()
        assert scene.render_view_rows_shade(view).tobytes() == fresh.render_view_rows_shade(view).tobytes()


def test_two_device_resident_rows_means_back_to_back_and_a_host_one_behind_them(rtx, torch, orc, bunny):
    view = bunny.own_view()
    w, h = ac.BUNNY_FRAME
    e7, e3, e8 = (ac.expected(orc, rtx, "bunny", n) for n in (7, 3, 8))
    side = torch.cuda.Stream()
    bufs = [(Guarded(torch, 16 * w * h), Guarded(torch, 16 * w * h), Guarded(torch, 3 * w * h, 1)) for _ in range(2)]
    torch.cuda.synchronize()
    for (d_acc, d_shade, d_rgb), n in zip(bufs, (7, 3)):
        bunny.render_view_mean_device(0, view, ac.SEEDS[:n], ac.N_PAIRS, d_acc.ptr, d_rgb.ptr, d_shade.ptr, side.cuda_stream, rows=True)
    rgb, shade = bunny.render_view_mean(view, ac.SEEDS[:8], ac.N_PAIRS, want_shade=True, rows=True)    # nothing waited for in between
    side.synchronize()
    check_mean(rgb, shade, e8, "host variant behind two device-resident calls")
    for (d_acc, d_shade, d_rgb), e in zip(bufs, (e7, e3)):
        check_mean(d_rgb.get().reshape(h, w, 3), d_shade.get(rtx.PIXEL_SHADE_DTYPE).reshape(h, w), e, "device-resident, side stream")
        assert ac.same_accum(d_acc.get(rtx.ACCUM_PIXEL_DTYPE).reshape(h, w), e["sum"], e["hit_frames"])


def expected_in(orc, frame, n_pairs, n):
    """accum_sets.expected's statement for the bunny in another frame under tables of another length: the oracle scene created
    with that frame (the same field of view) and the table gen_samples(SEEDS[k], n_pairs), frame by frame through the numpy
    statements"""
    w, h = frame
    acc = None
    for seed in ac.SEEDS[:n]:
        osc = orc.default_scene(["bunny.obj"], w, h, orc.gen_samples(seed, n_pairs), nb_light_sample=ac.BUNNY_LIGHT_SAMPLES, distance=6.0 * w)
        _, _, tri, lin = osc.render_rows(mode=orc.MODE_BVH, nthreads=4, want_tri=True, want_lin=True)
        osc.close()
        acc = ac.np_add(lin, tri != NO_HIT, acc)
    linear = ac.np_divide(acc[0], n)
    return dict(linear=linear, rgb8=ac.oracle_bytes(orc, linear), hits=np.minimum(acc[1], 255).astype(np.uint8), sum=acc[0], hit_frames=acc[1])


def test_the_three_mean_calls_share_a_scratch_that_grows_and_is_reused_smaller(rtx, torch, orc):
    """All three go through one path and share the scratch table and records.  On one side stream, nothing waited for: a
    view-kernel mean, a pipeline mean in a larger frame under a longer table (both scratch buffers grow), an adaptive mean
    under a rule that never stops and the view-kernel mean again, both back in the small frame under the short table; behind
    them a host pipeline mean.  The scene's own table (1000 pairs) lies between the two lengths."""
    n, small, large = 3, ((16, 12), 701), ((24, 16), 5003)
    seeds = ac.SEEDS[:n]
    e = {shape: expected_in(orc, *shape, n) for shape in (small, large)}
    for x in e.values():
        assert (x["hits"] == 0).any() and (x["hits"] == n).any()
    side = torch.cuda.Stream()
    s = side.cuda_stream
    with ac.open_bunny(rtx, ac.table(orc, 0)[:1000]) as scene:
        view = {shape: rtx.Scene.view(*shape[0], rtx.DEFAULT_EYE, rtx.DEFAULT_LOOK_AT, distance=6.0 * shape[0][0]) for shape in (small, large)}

        def buffers(shape, state_bytes):
            w, h = shape[0]
            return Guarded(torch, state_bytes * w * h), Guarded(torch, 16 * w * h), Guarded(torch, 3 * w * h, 1)

        calls = [("view", small, buffers(small, 16)), ("rows", large, buffers(large, 16)), ("adaptive", small, buffers(small, 32)),
                 ("view", small, buffers(small, 16))]
        d_tiles = Guarded(torch, 8 * 2 * 2)
        torch.cuda.synchronize()
        for how, shape, (d_state, d_shade, d_rgb) in calls:
            if how == "adaptive":
                scene.render_view_adaptive_device(0, view[shape], seeds, (n, 0.0), shape[1], d_state.ptr, d_tiles.ptr, d_rgb.ptr, d_shade.ptr, s)
            else:
                scene.render_view_mean_device(0, view[shape], seeds, shape[1], d_state.ptr, d_rgb.ptr, d_shade.ptr, s, rows=how == "rows")
        rgb, shade = scene.render_view_mean(view[small], seeds, small[1], want_shade=True, rows=True)
        side.synchronize()
        check_mean(rgb, shade, e[small], "host pipeline mean behind the four")
        for k, (how, shape, (d_state, d_shade, d_rgb)) in enumerate(calls):
            w, h = shape[0]
            check_mean(d_rgb.get().reshape(h, w, 3), d_shade.get(rtx.PIXEL_SHADE_DTYPE).reshape(h, w), e[shape], "call %d, %s" % (k, how))
            state = d_state.get(rtx.MOMENT_PIXEL_DTYPE if how == "adaptive" else rtx.ACCUM_PIXEL_DTYPE).reshape(h, w)
            assert ac.same_accum(state, e[shape]["sum"], e[shape]["hit_frames"]), "call %d, %s: the sums" % (k, how)
            if how == "adaptive":
                assert (state["frames"] == n).all() and (d_tiles.get(rtx.TILE_STATE_DTYPE)["frames"] == n).all()
