"""GPU parity of the adaptive mean through the render pipeline: rtx_render_view_rows_adaptive in both variants against the
expected values of tests/rows_adapt_sets.py — the oracle scene created with each frame's table, through adapt_sets' numpy
statements: moments, tile states with their stop frames, records and bytes — and against rtx_render_view_adaptive_device for
the same arguments, word for word; and the building block, rtx_render_view_rows_shade_masked_device, with hand-made tile
states against the unmasked record launch.  Every comparison is for equal bits or bytes (a NaN the statement makes stands for
any NaN)."""
import importlib
import os

import numpy as np
import pytest

import accum_sets as ac
import adapt_sets as ad
import gpu_forms as gf
import light_sets as ls
import prims_sets as pm
import resample_sets as rs
import rows_adapt_sets as ra
import view_sets as vs
from query_sets import F, bits

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 16
INF = float("inf")
NAN_WORD = 0x7FC0A5A5                        # what a stopped tile's records hold before a masked launch, and after it
NONE = 0xFFFFFFFF
BLOCK_RULE = (2, float(F(1e-3)))
# hand-made states under BLOCK_RULE: stopped; live for want of frames; live for its error; a NaN error loses the comparison
STOPPED, LIVE = (5, 0.0), ((1, 0.0), (5, 1.0), (7, float("nan")))


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


@pytest.fixture(scope="module")
def narrow(rtx, orc):
    with ra.open_narrow(rtx, ac.table(orc, 0)) as scene:
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


def check_adaptive(got_rgb, got_shade, got_tiles, e, what):
    assert np.array_equal(got_tiles["frames"], e["tiles"]["frames"]), "%s: tile frames\n%s\nexpected\n%s" % (what, got_tiles["frames"], e["tiles"]["frames"])
    assert np.array_equal(bits(got_tiles["err"]), bits(e["tiles"]["err"])), what + ": tile errors differ"
    assert np.array_equal(bits(got_shade["linear"]), bits(e["linear"])), "%s: %d pixels' linear words differ" % (
        what, (bits(got_shade["linear"]) != bits(e["linear"])).any(axis=-1).sum())
    assert np.array_equal(got_shade["rgb8"], e["rgb8"]), "%s: %d pixels' bytes differ" % (what, (got_shade["rgb8"] != e["rgb8"]).any(axis=-1).sum())
    assert np.array_equal(got_shade["hits"], e["hits"]), what + ": hits differ"
    if got_rgb is not None:
        assert np.array_equal(got_rgb, e["rgb8"]), what + ": out_rgb is not the records' bytes"


def adaptive_on_device(rtx, torch, scene, view, seeds, rule, n_pairs=ac.N_PAIRS, rgb_offset=1, state=None, stream=None, rows=True, **kw):
    """rtx_render_view_rows_adaptive_device (rows=False: the view kernel's rtx_render_view_adaptive_device) into guarded
    buffers -> (rgb, shade, tiles, moments, (d_mom, d_tiles)); state: an earlier call's buffers, to continue"""
    h, w = view.ny, view.nx
    ty, tx = ad.tile_grid(w, h)[::-1]
    d_mom, d_tiles = state if state else (Guarded(torch, 32 * w * h), Guarded(torch, 8 * tx * ty))
    d_shade, d_rgb = Guarded(torch, 16 * w * h), Guarded(torch, 3 * w * h, rgb_offset)
    call = scene.render_view_rows_adaptive_device if rows else scene.render_view_adaptive_device
    call(0, view, seeds, rule, n_pairs, d_mom.ptr, d_tiles.ptr, d_rgb.ptr, d_shade.ptr, stream if stream is not None else stream_of(torch),
         resume=state is not None, **kw)
    if stream is not None:
        return d_rgb, d_shade, d_tiles, d_mom
    return (d_rgb.get().reshape(h, w, 3), d_shade.get(rtx.PIXEL_SHADE_DTYPE).reshape(h, w), d_tiles.get(rtx.TILE_STATE_DTYPE).reshape(ty, tx),
            d_mom.get(rtx.MOMENT_PIXEL_DTYPE).reshape(h, w), (d_mom, d_tiles))


def same_as_the_view_kernels(rows, view_call, what):
    """two adaptive_on_device answers, word for word: bytes, records, tile states, moments"""
    for k, name in enumerate(("rgb", "records", "tile states", "moments")):
        assert rows[k].tobytes() == view_call[k].tobytes(), "%s: %s differ from rtx_render_view_adaptive_device's" % (what, name)


# ---------------------------------------------------------------------------------------------- 1: the fixtures
@pytest.mark.parametrize("fixture", ("bunny", "rows_low", "rows_mid", "rows_sky", "narrow"))
def test_the_windows_adaptive_mean_is_the_expected_record(rtx, torch, orc, bunny, narrow, fixture):
    scene = narrow if fixture == "narrow" else bunny
    e = ra.expected(orc, rtx, fixture)
    view = ra.view_of(rtx, scene, fixture)
    rule = ra.fixture_rule(fixture)
    rgb, shade, tiles, st = scene.render_view_rows_adaptive(view, ac.SEEDS, rule, ac.N_PAIRS, want_shade=True, want_tiles=True, stats=True)
    check_adaptive(rgb, shade, tiles, e, fixture + ", host variant")
    assert np.array_equal(np.where(ad.np_stopped(rule, tiles), tiles["frames"], 0), e["stop"])
    # the statistics: sums over the rendered tile-frames, read from the tile states; a stopped tile touches no counter
    pixel_frames, hits = int(e["mom"]["frames"].sum()), int(e["mom"]["hit_frames"].sum())
    print("%s: %d of %d pixel-frames rendered, %d hits" % (fixture, pixel_frames, ad.N_FRAMES * view.nx * view.ny, hits))
    assert st["primary_rays"] == pixel_frames and st["primary_hits"] == hits and st["shadow_rays"] == hits * ac.BUNNY_LIGHT_SAMPLES
    assert st["kernel_ms"] > 0 and pixel_frames < ad.N_FRAMES * view.nx * view.ny
    rgb2, shade2 = scene.render_view_rows_adaptive(view, ac.SEEDS, rule, ac.N_PAIRS, want_shade=True)      # uncounted
    assert shade2.tobytes() == shade.tobytes() and np.array_equal(rgb2, rgb)
    assert np.array_equal(scene.render_view_rows_adaptive(view, ac.SEEDS, rule, ac.N_PAIRS), e["rgb8"])     # rgb alone
    got = adaptive_on_device(rtx, torch, scene, view, ac.SEEDS, rule)
    check_adaptive(got[0], got[1], got[2], e, fixture + ", device variant")
    assert ad.same_moments(got[3], e["mom"])
    same_as_the_view_kernels(got, adaptive_on_device(rtx, torch, scene, view, ac.SEEDS, rule, rows=False), fixture)
    # the view-kernel call's host variant too
    v_rgb, v_shade, v_tiles = scene.render_view_adaptive(view, ac.SEEDS, rule, ac.N_PAIRS, want_shade=True, want_tiles=True)
    assert v_shade.tobytes() == shade.tobytes() and v_tiles.tobytes() == tiles.tobytes() and np.array_equal(v_rgb, rgb)


def test_the_yards_adaptive_mean_unposed_and_posed(rtx, torch, orc):
    """two rays per pixel (the passes of a frame hand on sums and hit counts; a stopped tile is skipped in both), spheres, a pose"""
    view = ac.yard_view(rtx)
    seeds = ac.SEEDS[:ac.YARD_FRAMES]
    with rs.open_yard(rtx, ac.table(orc, 3)) as scene:
        with pytest.raises(rtx.RtxError) as refused:                     # a posed call on a device without a pose
            scene.render_view_rows_adaptive(view, seeds, ad.YARD_RULE, ac.N_PAIRS, posed=True)
        assert refused.value.code == rtx.ERR_BAD_ARG
        scene.pose_prims(**pm.given(rtx, ac.YARD_POSE[1]))
        for fixture, posed in (("yard", False), ("yard_posed", True), ("yard", False)):
            e = ra.expected(orc, rtx, fixture)
            rgb, shade, tiles, st = scene.render_view_rows_adaptive(view, seeds, ad.YARD_RULE, ac.N_PAIRS, posed=posed, want_shade=True,
                                                                    want_tiles=True, stats=True)
            check_adaptive(rgb, shade, tiles, e, fixture + ", host variant")
            assert st["primary_rays"] == int(e["mom"]["frames"].sum()) * pm.NB_RAY
            got = adaptive_on_device(rtx, torch, scene, view, seeds, ad.YARD_RULE, rgb_offset=2, posed=posed)
            check_adaptive(got[0], got[1], got[2], e, fixture + ", device variant")
            assert ad.same_moments(got[3], e["mom"])
            same_as_the_view_kernels(got, adaptive_on_device(rtx, torch, scene, view, seeds, ad.YARD_RULE, rgb_offset=2, posed=posed, rows=False),
                                     fixture)


def test_a_given_light(rtx, torch, orc, bunny):
    """far_side with a count of seven against the oracle's frames under it; then the scene's own light, given"""
    tri, count = ls.SIDE_LIGHTS["far_side"][0], 7
    lins, hits = [], []
    for k in range(4):
        osc = orc.default_scene(["bunny.obj"], ac.BUNNY_FRAME[0], ac.BUNNY_FRAME[1], ac.table(orc, k), light_tri=tri, nb_light_sample=count)
        _, _, prim, lin = osc.render_rows(mode=orc.MODE_BVH, want_tri=True, want_lin=True)
        osc.close()
        lins.append(lin)
        hits.append(prim != 0xFFFFFFFF)
    rule = (2, float(F(3.1e-6)))             # 8 % from the nearest tile error (measured with the oracle): tiles stop at 2, 3, 4 and never
    e = ad.run(rule, lins, hits)
    e["linear"] = ad.np_divide_own(e["mom"])
    e["rgb8"] = ac.oracle_bytes(orc, e["linear"])
    e["hits"] = np.minimum(e["mom"]["hit_frames"], 255).astype(np.uint8)
    assert (e["stop"] == 0).any() and (e["stop"] > 2).any()
    light = rtx.Scene.make_light(tri, count)
    view = bunny.own_view()
    rgb, shade, tiles, st = bunny.render_view_rows_adaptive(view, ac.SEEDS[:4], rule, ac.N_PAIRS, light=light, want_shade=True,
                                                            want_tiles=True, stats=True)
    check_adaptive(rgb, shade, tiles, e, "far_side x 7, host variant")
    assert st["shadow_rays"] == 7 * st["primary_hits"]
    got = adaptive_on_device(rtx, torch, bunny, view, ac.SEEDS[:4], rule, light=light)
    check_adaptive(got[0], got[1], got[2], e, "far_side x 7, device variant")
    same_as_the_view_kernels(got, adaptive_on_device(rtx, torch, bunny, view, ac.SEEDS[:4], rule, light=light, rows=False), "far_side x 7")
    own = bunny.light()
    own.nb_light_sample = 0
    rgb, shade, tiles = bunny.render_view_rows_adaptive(view, ac.SEEDS, ad.RULE, ac.N_PAIRS, light=own, want_shade=True, want_tiles=True)
    check_adaptive(rgb, shade, tiles, ra.expected(orc, rtx, "bunny"), "the scene's own light, given")


# ---------------------------------------------------------------------------------------------- 2: the equivalences
@pytest.mark.parametrize("n", (1, 3, 8))
def test_a_rule_that_never_stops_is_the_rows_mean(rtx, torch, bunny, n):
    """min_frames = n_frames: outputs and the sum / hit_frames words equal rtx_render_view_rows_mean_device's"""
    view = bunny.own_view()
    w, h = ac.BUNNY_FRAME
    d_acc, m_shade, m_rgb = Guarded(torch, 16 * w * h), Guarded(torch, 16 * w * h), Guarded(torch, 3 * w * h, 1)
    bunny.render_view_mean_device(0, view, ac.SEEDS[:n], ac.N_PAIRS, d_acc.ptr, m_rgb.ptr, m_shade.ptr, stream_of(torch), rows=True)
    d_rgb, d_shade, d_tiles, d_mom, _ = adaptive_on_device(rtx, torch, bunny, view, ac.SEEDS[:n], (n, 0.0))
    acc = d_acc.get(rtx.ACCUM_PIXEL_DTYPE).reshape(h, w)
    assert np.array_equal(bits(d_mom["sum"]), bits(acc["sum"])) and np.array_equal(d_mom["hit_frames"], acc["hit_frames"])
    assert (d_mom["frames"] == n).all() and (d_tiles["frames"] == n).all()
    assert d_shade.tobytes() == m_shade.get(rtx.PIXEL_SHADE_DTYPE).reshape(h, w).tobytes()
    assert np.array_equal(d_rgb, m_rgb.get().reshape(h, w, 3))
    rgb, shade = bunny.render_view_rows_adaptive(view, ac.SEEDS[:n], (n, INF), ac.N_PAIRS, want_shade=True)
    m = bunny.render_view_mean(view, ac.SEEDS[:n], ac.N_PAIRS, want_shade=True, rows=True)
    assert shade.tobytes() == m[1].tobytes() and np.array_equal(rgb, m[0])


def test_min_frames_of_one_is_the_one_frame_mean(rtx, torch, bunny):
    """the trap the header names: after one frame the variance is exactly 0, so every tile stops for any threshold — four
    frames in which the masked launch schedules nothing"""
    view = bunny.own_view()
    m_rgb, m_shade = bunny.render_view_mean(view, ac.SEEDS[:1], ac.N_PAIRS, want_shade=True, rows=True)
    for max_variance in (0.0, INF):
        rgb, shade, tiles, st = bunny.render_view_rows_adaptive(view, ac.SEEDS[:5], (1, max_variance), ac.N_PAIRS, want_shade=True,
                                                                want_tiles=True, stats=True)
        assert shade.tobytes() == m_shade.tobytes() and np.array_equal(rgb, m_rgb)
        assert (tiles["frames"] == 1).all() and (bits(tiles["err"]) == 0).all()
        assert st["primary_rays"] == view.nx * view.ny and st["primary_hits"] == int((m_shade["hits"] != 0).sum())
    descs = descs_of(bunny, view)                                       # the last frame's launch: nothing scheduled
    assert (descs[:, :, 0] == NONE).all() and not descs[:, :, 1:].any()


def test_three_and_five_frames_are_eight(rtx, torch, orc, bunny):
    view = bunny.own_view()
    e = ra.expected(orc, rtx, "bunny")
    *_, state = adaptive_on_device(rtx, torch, bunny, view, ac.SEEDS[:3], ad.RULE)
    three = ra.expected(orc, rtx, "bunny", 3)
    assert ad.same_moments(state[0].get(rtx.MOMENT_PIXEL_DTYPE).reshape(three["stop"].shape[0] * 8, -1), three["mom"])
    d_rgb, d_shade, d_tiles, d_mom, _ = adaptive_on_device(rtx, torch, bunny, view, ac.SEEDS[3:], ad.RULE, state=state)
    check_adaptive(d_rgb, d_shade, d_tiles, e, "3 + 5 frames")
    assert ad.same_moments(d_mom, e["mom"])
    whole = adaptive_on_device(rtx, torch, bunny, view, ac.SEEDS, ad.RULE)
    assert whole[3].tobytes() == d_mom.tobytes() and whole[2].tobytes() == d_tiles.tobytes() and whole[1].tobytes() == d_shade.tobytes()


def test_a_stricter_rule_resumes_stopped_tiles(rtx, torch, orc, bunny):
    view = bunny.own_view()
    lins, hits = ad.fixture_frames(orc, rtx, "bunny", ad.N_FRAMES)
    first = ad.run(ad.RULE, lins[:4], hits[:4])
    strict = (2, float(F(3e-7)))
    e = ad.run(strict, lins[4:], hits[4:], state=(first["mom"], first["tiles"]))
    resumed = (first["stop"] != 0) & (e["tiles"]["frames"] > first["tiles"]["frames"])
    still = (first["stop"] != 0) & (e["tiles"]["frames"] == first["tiles"]["frames"])
    assert resumed.sum() >= 2 and still.sum() >= 2                       # the lit ground resumes, the sky (error 0) does not
    e["linear"] = ad.np_divide_own(e["mom"])
    e["rgb8"] = ac.oracle_bytes(orc, e["linear"])
    e["hits"] = np.minimum(e["mom"]["hit_frames"], 255).astype(np.uint8)
    *_, state = adaptive_on_device(rtx, torch, bunny, view, ac.SEEDS[:4], ad.RULE)
    d_rgb, d_shade, d_tiles, d_mom, _ = adaptive_on_device(rtx, torch, bunny, view, ac.SEEDS[4:], strict, state=state)
    check_adaptive(d_rgb, d_shade, d_tiles, e, "4 frames, then 4 under a stricter rule")
    assert ad.same_moments(d_mom, e["mom"])


# ---------------------------------------------------------------------------------------------- 3: the building block
def block_states(rtx, tiles_x, tiles_y, stopped):
    """hand-made states for a bool [tiles_y, tiles_x]: STOPPED where set, the LIVE kinds in turn elsewhere"""
    st = np.zeros((tiles_y, tiles_x), rtx.TILE_STATE_DTYPE)
    k = 0
    for ty in range(tiles_y):
        for tx in range(tiles_x):
            st[ty, tx] = STOPPED if stopped[ty, tx] else LIVE[k % len(LIVE)]
            k += not stopped[ty, tx]
    assert np.array_equal(ad.np_stopped(BLOCK_RULE, st), stopped)
    return st


def checkerboard(tiles_x, tiles_y, phase=0):
    return (np.add.outer(np.arange(tiles_y), np.arange(tiles_x)) + phase) % 2 == 0


def masked_launch(rtx, torch, scene, view, states, rule=BLOCK_RULE, counted=False, **kw):
    """rtx_render_view_rows_shade_masked_device over records pre-filled with NAN_WORD, guard bytes behind them and behind the
    states -> (records [ny, width] as uint32 words [ny, width, 4], the eight counters or None)"""
    ny, w = view.ny, view.width
    d_shade = Guarded(torch, 16 * ny * w).put(np.full(4 * ny * w, NAN_WORD, np.uint32))
    d_tiles = Guarded(torch, states.nbytes).put(states)
    counters = torch.zeros(8, dtype=torch.int64, device="cuda:0") if counted else None
    scene.render_view_rows_shade_masked_device(0, view, d_tiles.ptr, rule, d_shade.ptr, 16 * ny * w, stream_of(torch),
                                               counters.data_ptr() if counted else None, **kw)
    words = d_shade.get(np.uint32).reshape(ny, w, 4)
    assert d_tiles.get().tobytes() == states.tobytes()                  # the launch reads the states only
    return words, (counters.cpu().numpy().astype(np.uint64) if counted else None)


def unmasked_counters(torch, scene, view, **kw):
    ny, w = view.ny, view.width
    d_shade = Guarded(torch, 16 * ny * w)
    counters = torch.zeros(8, dtype=torch.int64, device="cuda:0")
    scene.render_view_rows_shade_device(0, view, d_shade.ptr, 16 * ny * w, stream_of(torch), counters.data_ptr(), **kw)
    d_shade.get()
    return counters.cpu().numpy().astype(np.uint64)


def check_block(rtx, scene, view, words, stopped, want, what):
    """stopped tiles keep the pattern, live tiles equal the unmasked launch's records; the descriptors of the launch show
    unscheduled tiles exactly where a tile was stopped, and the unmasked launch's elsewhere"""
    ny, w = view.ny, view.width
    tiles_x, tiles_y = ad.tile_grid(w, ny)
    px = ad.tiles_of(stopped)[:ny, :w]
    assert (words[px] == NAN_WORD).all(), "%s: %d words of stopped tiles were written" % (what, (words[px] != NAN_WORD).sum())
    got = np.ascontiguousarray(words).view(rtx.PIXEL_SHADE_DTYPE).reshape(ny, w)
    live = ~px
    assert np.array_equal(got["hits"][live], want["hits"][live]) and np.array_equal(got["rgb8"][live], want["rgb8"][live]), what
    gl, wl = got["linear"][live], want["linear"][live]
    nan = np.isnan(wl)
    assert np.array_equal(np.isnan(gl), nan) and np.array_equal(bits(gl)[~nan], bits(wl)[~nan]), what + ": live tiles' linear words"
    return got


def descs_of(scene, view, stopped=None):
    """tile_descs of the most recent launch as [tiles_y, tiles_x, 4] (the pipeline's numbering undone)"""
    tiles_x, tiles_y = ad.tile_grid(view.width, view.ny)
    d = scene.tile_descs()
    assert len(d) == ((tiles_x + 7) // 8) * ((tiles_y + 7) // 8) * 64
    return np.array([[d[ra.swizzled_tile_id(tx, ty, tiles_x)] for tx in range(tiles_x)] for ty in range(tiles_y)])


def check_descs(masked, plain, stopped, what, with_hits=True):
    assert (masked[stopped][:, 0] == NONE).all() and not masked[stopped][:, 1:].any(), what + ": a stopped tile's descriptor"
    assert np.array_equal(masked[~stopped][:, :3], plain[~stopped][:, :3]), what + ": a live tile's descriptor"
    if with_hits:
        assert (plain[stopped][:, 1] > 0).any() and (plain[stopped][:, 0] != NONE).any(), what + ": no stopped tile was scheduled before"


def test_a_checkerboard_of_stopped_tiles(rtx, torch, orc, bunny):
    """6 x 4 tiles; every other tile stopped, then the other half; all live; all stopped; rows off the tile grid"""
    for view in (bunny.own_view(), ra.view_of(rtx, bunny, "rows_low")):
        tiles_x, tiles_y = ad.tile_grid(view.width, view.ny)
        want = bunny.render_view_rows_shade(view)
        plain = descs_of(bunny, view)
        for name, stopped in (("even", checkerboard(tiles_x, tiles_y)), ("odd", checkerboard(tiles_x, tiles_y, 1)),
                              ("none", np.zeros((tiles_y, tiles_x), bool)), ("all", np.ones((tiles_y, tiles_x), bool))):
            words, _ = masked_launch(rtx, torch, bunny, view, block_states(rtx, tiles_x, tiles_y, stopped))
            check_block(rtx, bunny, view, words, stopped, want, name)
            if stopped.any():
                check_descs(descs_of(bunny, view), plain, stopped, name)
        # under another light, and the rule decides: the same states under a rule that stops nothing
        light = rtx.Scene.make_light(ls.SIDE_LIGHTS["far_side"][0], 7)
        stopped = checkerboard(tiles_x, tiles_y)
        words, _ = masked_launch(rtx, torch, bunny, view, block_states(rtx, tiles_x, tiles_y, stopped), light=light)
        check_block(rtx, bunny, view, words, stopped, bunny.render_view_rows_shade(view, light=light), "far_side x 7")
        words, _ = masked_launch(rtx, torch, bunny, view, block_states(rtx, tiles_x, tiles_y, stopped), rule=(6, 0.0))
        check_block(rtx, bunny, view, words, np.zeros_like(stopped), want, "a rule that stops none of these states")
    # the scene's other calls are what they were
    assert np.array_equal(bunny.render_view_rows_shade(bunny.own_view())["rgb8"], bunny.render_view_rows(bunny.own_view()))
    assert np.array_equal(bunny.render_rows(), bunny.render_view_rows(bunny.own_view()))


def test_nine_by_nine_tiles_cross_a_block_of_the_numbering(rtx, torch, orc):
    """a 72 x 70 bunny frame: 9 x 9 tiles, so the pipeline's tile number crosses a block of 8 x 8 tiles in both directions
    and differs from the states' row-major number almost everywhere; the bottom edge is ragged (70 = 8 * 8 + 6)"""
    with rtx.default_scene([os.path.join(ROOT, "models", "bunny.obj")], 72, 70, ac.table(orc, 0), nb_light_sample=4) as scene:
        view = scene.own_view()
        tiles_x, tiles_y = ad.tile_grid(72, 70)
        assert (tiles_x, tiles_y) == (9, 9)
        want = scene.render_view_rows_shade(view)
        plain = descs_of(scene, view)
        rng = np.random.default_rng(20261023)
        for name, stopped in (("even", checkerboard(9, 9)), ("odd", checkerboard(9, 9, 1)), ("random", rng.random((9, 9)) < 0.5),
                              ("the last row and column alone live", np.logical_and.outer(np.arange(9) < 8, np.arange(9) < 8))):
            words, _ = masked_launch(rtx, torch, scene, view, block_states(rtx, 9, 9, stopped))
            check_block(rtx, scene, view, words, stopped, want, name)
            check_descs(descs_of(scene, view), plain, stopped, name)
        before = (scene.render_view_rows(view).tobytes(), scene.render_rows().tobytes(), scene.render_view_rows_shade(view).tobytes())
        masked_launch(rtx, torch, scene, view, block_states(rtx, 9, 9, checkerboard(9, 9)))
        assert (scene.render_view_rows(view).tobytes(), scene.render_rows().tobytes(), scene.render_view_rows_shade(view).tobytes()) == before


@pytest.mark.parametrize("n_spheres", [0, 40])
def test_the_whole_stream_forms(rtx, torch, samples_seeded, n_spheres):
    """a scene too large to cut per tile: the WHOLE forms, two rays per pixel — a stopped tile is skipped in both passes of
    the frame and writes no word of the sums and hit counts the passes hand on"""
    tris, rgb, extra = gf.whole_stream_scene(rtx, n_spheres=n_spheres)
    with rtx.Scene(24, 24, tris, rgb, samples_seeded, nb_ray=2, nb_light_sample=4, leaf_max=1, reference_tree=rtx.REFTREE_NEVER,
                   tie_rank=None, **extra) as scene:
        assert scene.info()["n_nodes"] > gf.CUT_MAX_NODES
        view = scene.own_view()
        want = scene.render_view_rows_shade(view)
        plain = descs_of(scene, view)
        for phase in (0, 1):
            stopped = checkerboard(3, 3, phase)
            words, _ = masked_launch(rtx, torch, scene, view, block_states(rtx, 3, 3, stopped))
            check_block(rtx, scene, view, words, stopped, want, "whole stream, phase %d" % phase)
            check_descs(descs_of(scene, view), plain, stopped, "whole stream")
        assert want["hits"].max() == 2
        words, ctr = masked_launch(rtx, torch, scene, view, block_states(rtx, 3, 3, stopped), counted=True)      # the counted WHOLE forms
        check_block(rtx, scene, view, words, stopped, want, "whole stream, counted")
        # (a descriptor's spare word: the hits the tile counted over the frame's passes)
        assert int(ctr[0]) == int(plain[~stopped][:, 3].sum()) > 0 and int(ctr[5]) == 0


def test_counters_are_the_live_tiles(rtx, torch, orc, bunny):
    """the COUNT forms.  A stopped tile touches no counter.  Exact for every mask: the primary hits (the sum of the live
    tiles' hits of an unmasked launch's descriptors), the tiles re-rendered, and the scheduling pass's own record fetches
    (counters 6, 7: a tile's primary walk does not depend on the other tiles) — a mask and its complement add up to the
    unmasked launch, once the padding is taken off: the tiles that pad the numbering's blocks of 8 x 8 (40 of 64 here) have no
    state and no pixel, run in every launch as they do in the unmasked one, and each fetches the root's record for no ray;
    a launch with every tile stopped counts exactly those.  The shading pass's test and fetch counts (1 .. 4) depend on how the order pass cuts a tile into parts,
    which depends on the launch's total cost, so they are exact where the launch is the same: every tile live."""
    view = bunny.own_view()
    tiles_x, tiles_y = ad.tile_grid(view.width, view.ny)
    whole = unmasked_counters(torch, bunny, view)
    plain = descs_of(bunny, view)
    want = bunny.render_view_rows_shade(view)
    none = np.zeros((tiles_y, tiles_x), bool)
    words, all_live = masked_launch(rtx, torch, bunny, view, block_states(rtx, tiles_x, tiles_y, none), counted=True)
    check_block(rtx, bunny, view, words, none, want, "counted, every tile live")
    print("unmasked %s\nall live %s" % (whole.tolist(), all_live.tolist()))
    assert np.array_equal(all_live, whole)
    _, all_stopped = masked_launch(rtx, torch, bunny, view, block_states(rtx, tiles_x, tiles_y, ~none), counted=True)
    padding = 64 - tiles_x * tiles_y
    assert not all_stopped[[0, 1, 2, 5]].any() and (all_stopped[[3, 4, 6, 7]] == padding * (whole[6] // 64)).all(), all_stopped.tolist()
    assert whole[6] % 64 == 0
    for phase in (0, 1):
        stopped = checkerboard(tiles_x, tiles_y, phase)
        words, a = masked_launch(rtx, torch, bunny, view, block_states(rtx, tiles_x, tiles_y, stopped), counted=True)
        check_block(rtx, bunny, view, words, stopped, want, "counted")
        _, b = masked_launch(rtx, torch, bunny, view, block_states(rtx, tiles_x, tiles_y, ~stopped), counted=True)
        print("phase %d: %s + %s" % (phase, a.tolist(), b.tolist()))
        assert int(a[0]) == int(plain[~stopped][:, 1].sum()) and int(b[0]) == int(plain[stopped][:, 1].sum())
        for k in (0, 5, 6, 7):
            assert int(a[k]) + int(b[k]) == int(whole[k]) + int(all_stopped[k]), k
        assert (a[1:5] > 0).all() and (b[1:5] > 0).all()


def test_a_tile_that_holds_a_negative_zero_ray(rtx, torch, orc, samples_seeded):
    """view_sets' scene P through its description's axis camera: the centre row's -0.0 direction components queue their
    tiles for the reference pass in the SCHEDULING pass.  Stopped, such a tile is not queued and its records are untouched;
    live, it equals the unmasked launch through the reference pass"""
    hs = vs.hard_scene("P", orc, samples_seeded, rtx)
    with rtx.Scene(*hs["args"], **hs["kw"]) as scene:
        (w, h) = hs["v"][0]
        view = rtx.Scene.view(w, h, **vs.camera(hs["v"]))
        tiles_x, tiles_y = ad.tile_grid(w, h)
        whole = unmasked_counters(torch, scene, view)
        want = scene.render_view_rows_shade(view)
        plain = descs_of(scene, view)
        hard = (plain[:, :, 2] & 2) != 0                                 # queued by the unmasked launch
        assert hard.any() and not hard.all() and int(whole[5]) == int(hard.sum())
        words, ctr = masked_launch(rtx, torch, scene, view, block_states(rtx, tiles_x, tiles_y, hard), counted=True)
        check_block(rtx, scene, view, words, hard, want, "the hard tiles stopped")
        check_descs(descs_of(scene, view), plain, hard, "the hard tiles stopped", with_hits=False)      # (a queued tile states no hits)
        assert (plain[hard][:, 2] != 0).all()
        assert int(ctr[5]) == 0                                         # nothing was queued
        words, ctr = masked_launch(rtx, torch, scene, view, block_states(rtx, tiles_x, tiles_y, ~hard), counted=True)
        check_block(rtx, scene, view, words, ~hard, want, "the hard tiles alone live")
        assert int(ctr[5]) == int(hard.sum()) and np.array_equal(descs_of(scene, view)[hard][:, :3], plain[hard][:, :3])
        assert np.array_equal(scene.render_view_rows(view), hs["ref"]["frame"])      # and the scene's byte launch is what it was


# ---------------------------------------------------------------------------------------------- 4: state and ordering
def test_masked_launches_leave_the_scene_untouched(rtx, torch, orc):
    with rs.open_yard(rtx, ac.table(orc, 4)) as scene:
        view = scene.own_view()
        mean_view = ac.yard_view(rtx)

        def state():
            return (scene.debug_samples().tobytes(), scene.samples_at().tobytes(), scene.render_rows().tobytes(),
                    scene.render_view_rows(view).tobytes(), scene.render_view_rows_shade(view).tobytes(),
                    scene.debug_light_points(scene.light()).tobytes(), scene.info(),
                    scene.render_view_mean(mean_view, ac.SEEDS[:3], ac.N_PAIRS, want_shade=True, rows=True)[1].tobytes())

        before = state()
        scene.render_view_rows_adaptive(mean_view, ac.SEEDS[:3], ad.YARD_RULE, ac.N_PAIRS)
        adaptive_on_device(rtx, torch, scene, mean_view, ac.SEEDS[:3], ad.YARD_RULE, n_pairs=7001, light=rtx.Scene.make_light(*pm.POSE_LIGHT))
        tiles_x, tiles_y = ad.tile_grid(mean_view.width, mean_view.ny)
        masked_launch(rtx, torch, scene, mean_view, block_states(rtx, tiles_x, tiles_y, checkerboard(tiles_x, tiles_y)))
        assert state() == before
        sched, shade = scene.launch_timings()                           # a masked launch counts as a launch
        n = len(sched)
        masked_launch(rtx, torch, scene, mean_view, block_states(rtx, tiles_x, tiles_y, checkerboard(tiles_x, tiles_y)))
        torch.cuda.synchronize()
        sched, shade = scene.launch_timings()
        assert len(sched) == min(n + 1, 64) and sched[-1] > 0 and shade[-1] > 0


def test_device_resident_calls_on_a_stream_of_their_own_and_host_calls_behind_them(rtx, torch, orc, bunny):
    """device-resident launches on one device are ordered on one stream; the host entry points wait for the most recent of
    them by an event before they reuse the scratch table, the scratch records and the light buffers"""
    view = bunny.own_view()
    w, h = ac.BUNNY_FRAME
    e8, e3 = ra.expected(orc, rtx, "bunny"), ra.expected(orc, rtx, "bunny", 3)
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    bufs = [adaptive_on_device(rtx, torch, bunny, view, ac.SEEDS[:n], ad.RULE, stream=side.cuda_stream) for n in (8, 3)]
    m_rgb, m_shade = bunny.render_view_mean(view, ac.SEEDS[:7], ac.N_PAIRS, want_shade=True, rows=True)      # nothing waited for in between
    rgb, shade, tiles = bunny.render_view_rows_adaptive(view, ac.SEEDS, ad.RULE, ac.N_PAIRS, want_shade=True, want_tiles=True)
    side.synchronize()
    m = ac.expected(orc, rtx, "bunny", 7)
    assert np.array_equal(bits(m_shade["linear"]), bits(m["linear"])) and np.array_equal(m_rgb, m["rgb8"])
    check_adaptive(rgb, shade, tiles, e8, "host variant behind two device-resident calls")
    for (d_rgb, d_shade, d_tiles, d_mom), e in zip(bufs, (e8, e3)):
        check_adaptive(d_rgb.get().reshape(h, w, 3), d_shade.get(rtx.PIXEL_SHADE_DTYPE).reshape(h, w),
                       d_tiles.get(rtx.TILE_STATE_DTYPE).reshape(e["stop"].shape), e, "device-resident, side stream")
        assert ad.same_moments(d_mom.get(rtx.MOMENT_PIXEL_DTYPE).reshape(h, w), e["mom"])
