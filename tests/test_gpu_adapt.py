"""GPU parity of the adaptive mean of N frames: the building blocks (rtx_moment_add_device, rtx_moment_resolve_device)
against the host statements word for word, and rtx_render_view_adaptive in both variants against the expected values of
tests/adapt_sets.py — the oracle scene created with each frame's table, through the numpy statements: moments, tile states
with their stop frames, records and bytes — whose conditions tests/test_adapt_sets.py asserts without a GPU.  Every comparison
is for equal bits or bytes (a NaN the statement makes stands for any NaN: the host's and the device's default NaN need not be
the same word)."""
import importlib

import numpy as np
import pytest

import accum_sets as ac
import adapt_sets as ad
import light_sets as ls
import prims_sets as pm
import resample_sets as rs
from query_sets import F, bits

pytestmark = pytest.mark.gpu
GUARD = 16
INF = float("inf")


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


def n_tiles_of(nx, ny):
    tx, ty = ad.tile_grid(nx, ny)
    return tx * ty


def same_host_moments(got, want):
    """two MOMENT_PIXEL_DTYPE arrays, word for word, a NaN standing for any NaN"""
    return ad.same_moments(got, {k: want[k] for k in ("sum", "hit_frames", "sumsq", "frames")})


def rect_view(rtx, view, rect):
    v = rtx.rtx.RtxView.from_buffer_copy(view)
    v.x0, v.y0, v.nx, v.ny = rect
    return v


# ---------------------------------------------------------------------------------------------- 1: the building blocks
BLOCK_SHAPES = {"synthetic": ad.SYNTHETIC_SHAPE, "ragged": (13, 19), "1x1": (1, 1), "8x8": (8, 8), "9x8": (8, 9)}      # (ny, nx)


@pytest.mark.parametrize("name", sorted(BLOCK_SHAPES))
@pytest.mark.parametrize("with_tiles", (True, False))
def test_the_kernels_are_the_host_statements(rtx, torch, bunny, name, with_tiles):
    ny, nx = BLOCK_SHAPES[name]
    n = nx * ny
    thr = bunny.gamma_thresholds()
    syn = [rec[:ny, :nx] for rec in ad.synthetic(rtx)]
    rule = ad.SYNTHETIC_RULE if with_tiles else None
    d_mom = Guarded(torch, 32 * n)                                       # first over garbage: 0xAA bytes
    d_tiles = Guarded(torch, 8 * n_tiles_of(nx, ny))
    want = w_tiles = None
    for k, rec in enumerate(syn):
        d_rec = Guarded(torch, 16 * n).put(rec)
        bunny.moment_add_device(0, nx, ny, d_rec.ptr, d_mom.ptr, d_tiles.ptr if with_tiles else None, k == 0, rule, stream_of(torch))
        if with_tiles:
            want, w_tiles = rtx.moment_add(rec, rule=rule) if k == 0 else rtx.moment_add(rec, want, w_tiles, rule=rule)
            assert ad.same_tiles(d_tiles.get(rtx.TILE_STATE_DTYPE).reshape(w_tiles.shape), w_tiles), (name, k)
        else:
            want = rtx.moment_add(rec, want)
            assert (d_tiles.get() == 0xAA).all()                        # tiles == NULL: no state is written
        assert same_host_moments(d_mom.get(rtx.MOMENT_PIXEL_DTYPE).reshape(ny, nx), want), (name, k)
        assert d_rec.get(rtx.PIXEL_SHADE_DTYPE).tobytes() == rec.tobytes()                       # an add reads its records only
        if k == 0:
            assert np.array_equal(bits(d_mom.get(rtx.MOMENT_PIXEL_DTYPE)["sum"].reshape(ny, nx, 3)), bits(rec["linear"]))
    # ... and the host statements are the numpy statements (tests/test_adapt_host.py), so the device's words are the fixture's
    if name == "synthetic" and with_tiles:
        e = ad.synthetic_run(rtx)
        assert ad.same_moments(want, e["mom"]) and ad.same_tiles(w_tiles, e["tiles"]) and len(set(e["stop"].ravel().tolist())) >= 2
    w_rgb, w_shade = rtx.moment_resolve(thr, want)
    for offset in range(4):                                             # d_rgb at byte offsets 0, 1, 2, 3
        for with_rgb, with_shade in ((True, False), (False, True), (True, True)):
            d_rgb = Guarded(torch, 3 * n, offset) if with_rgb else None
            d_shade = Guarded(torch, 16 * n) if with_shade else None
            bunny.moment_resolve_device(0, n, d_mom.ptr, d_rgb.ptr if with_rgb else None, d_shade.ptr if with_shade else None,
                                        stream_of(torch))
            if with_rgb:
                assert np.array_equal(d_rgb.get().reshape(ny, nx, 3), w_rgb), (name, offset)
            if with_shade:
                assert ac.same_records(d_shade.get(rtx.PIXEL_SHADE_DTYPE).reshape(ny, nx), w_shade), (name, offset)
    assert same_host_moments(d_mom.get(rtx.MOMENT_PIXEL_DTYPE).reshape(ny, nx), want)             # a resolve reads its moments only


def test_a_stopped_tile_is_not_touched(rtx, torch, bunny):
    """once a tile has stopped, the next add is handed records full of NaN for it: its moments and its state keep their
    words; the live tiles beside it go on"""
    ny, nx = 13, 19
    rng = np.random.default_rng(20261022)
    rule = (2, float(F(2e-4)))

    def frame(noise):
        rec = np.zeros((ny, nx), rtx.PIXEL_SHADE_DTYPE)
        rec["linear"] = (F(0.5) + noise * (rng.random((ny, nx, 3)).astype(F) - F(0.5))).astype(F)
        rec["hits"] = 1
        return rec

    # the left column of tiles is quiet (stops at 2), the others are noisy (never stop under this rule)
    noise = np.where(np.arange(nx) < 8, F(1e-3), F(0.5)).astype(F)[None, :, None]
    d_mom, d_tiles = Guarded(torch, 32 * nx * ny), Guarded(torch, 8 * 6)
    want = w_tiles = None
    for k in range(2):
        rec = frame(noise)
        bunny.moment_add_device(0, nx, ny, Guarded(torch, 16 * nx * ny).put(rec).ptr, d_mom.ptr, d_tiles.ptr, k == 0, rule, stream_of(torch))
        want, w_tiles = rtx.moment_add(rec, rule=rule) if k == 0 else rtx.moment_add(rec, want, w_tiles, rule=rule)
    stopped = ad.np_stopped(rule, w_tiles)
    assert stopped.tolist() == [[True, False, False], [True, False, False]]
    before_mom, before_tiles = d_mom.get(rtx.MOMENT_PIXEL_DTYPE).reshape(ny, nx).copy(), d_tiles.get(rtx.TILE_STATE_DTYPE).reshape(2, 3).copy()
    assert ad.same_tiles(before_tiles, w_tiles) and same_host_moments(before_mom, want)
    for k in range(2):
        rec = frame(noise)
        rec["linear"][:, :8] = np.nan
        rec["hits"][:, :8] = 255
        bunny.moment_add_device(0, nx, ny, Guarded(torch, 16 * nx * ny).put(rec).ptr, d_mom.ptr, d_tiles.ptr, False, rule, stream_of(torch))
        rtx.moment_add(rec, want, w_tiles, rule=rule)
        got_mom, got_tiles = d_mom.get(rtx.MOMENT_PIXEL_DTYPE).reshape(ny, nx), d_tiles.get(rtx.TILE_STATE_DTYPE).reshape(2, 3)
        assert got_mom[:, :8].tobytes() == before_mom[:, :8].tobytes() and got_tiles[:, 0].tobytes() == before_tiles[:, 0].tobytes()
        assert not np.isnan(got_mom["sum"]).any() and (got_tiles["frames"][:, 1:] == 3 + k).all()
        assert ad.same_tiles(got_tiles, w_tiles) and same_host_moments(got_mom, want)
    # without tile states nothing is masked: the same records reach every pixel
    bunny.moment_add_device(0, nx, ny, Guarded(torch, 16 * nx * ny).put(rec).ptr, d_mom.ptr, None, False, None, stream_of(torch))
    assert np.isnan(d_mom.get(rtx.MOMENT_PIXEL_DTYPE).reshape(ny, nx)["sum"][:, :8]).all()


# ---------------------------------------------------------------------------------------------- 2: the adaptive call
def check_adaptive(got_rgb, got_shade, got_tiles, e, what):
    assert np.array_equal(got_tiles["frames"], e["tiles"]["frames"]), "%s: tile frames\n%s\nexpected\n%s" % (what, got_tiles["frames"], e["tiles"]["frames"])
    assert np.array_equal(bits(got_tiles["err"]), bits(e["tiles"]["err"])), what + ": tile errors differ"
    assert np.array_equal(bits(got_shade["linear"]), bits(e["linear"])), "%s: %d pixels' linear words differ" % (
        what, (bits(got_shade["linear"]) != bits(e["linear"])).any(axis=-1).sum())
    assert np.array_equal(got_shade["rgb8"], e["rgb8"]), "%s: %d pixels' bytes differ" % (what, (got_shade["rgb8"] != e["rgb8"]).any(axis=-1).sum())
    assert np.array_equal(got_shade["hits"], e["hits"]), what + ": hits differ"
    if got_rgb is not None:
        assert np.array_equal(got_rgb, e["rgb8"]), what + ": out_rgb is not the records' bytes"


def adaptive_on_device(rtx, torch, scene, view, seeds, rule, n_pairs=ac.N_PAIRS, rgb_offset=1, state=None, stream=None, **kw):
    """rtx_render_view_adaptive_device into guarded buffers -> (rgb, shade, tiles, moments, (d_mom, d_tiles)); state: an
    earlier call's buffers, to continue"""
    h, w = view.ny, view.nx
    ty, tx = ad.tile_grid(w, h)[::-1]
    d_mom, d_tiles = state if state else (Guarded(torch, 32 * w * h), Guarded(torch, 8 * tx * ty))
    d_shade, d_rgb = Guarded(torch, 16 * w * h), Guarded(torch, 3 * w * h, rgb_offset)
    scene.render_view_adaptive_device(0, view, seeds, rule, n_pairs, d_mom.ptr, d_tiles.ptr, d_rgb.ptr, d_shade.ptr,
                                      stream if stream is not None else stream_of(torch), resume=state is not None, **kw)
    if stream is not None:
        return d_rgb, d_shade, d_tiles, d_mom
    return (d_rgb.get().reshape(h, w, 3), d_shade.get(rtx.PIXEL_SHADE_DTYPE).reshape(h, w), d_tiles.get(rtx.TILE_STATE_DTYPE).reshape(ty, tx),
            d_mom.get(rtx.MOMENT_PIXEL_DTYPE).reshape(h, w), (d_mom, d_tiles))


def rendered(e, n_frames):
    """(pixel-frames, hits) of the rendered tile-frames of an expected run: frame k reaches the tiles that had not stopped
    after frame k - 1"""
    return int(e["mom"]["frames"].sum()), int(e["mom"]["hit_frames"].sum())


@pytest.mark.parametrize("fixture", ("bunny", "ragged", "ragged_low"))
def test_the_bunnys_adaptive_mean_is_the_expected_record(rtx, torch, orc, bunny, fixture):
    e = ad.expected(orc, rtx, fixture)
    view = bunny.own_view()
    if fixture != "bunny":
        view = rect_view(rtx, view, ad.RAGGED_RECT if fixture == "ragged" else ad.RAGGED_LOW_RECT)
    rgb, shade, tiles, st = bunny.render_view_adaptive(view, ac.SEEDS, ad.RULE, ac.N_PAIRS, want_shade=True, want_tiles=True, stats=True)
    check_adaptive(rgb, shade, tiles, e, fixture + ", host variant")
    assert np.array_equal(np.where(ad.np_stopped(ad.RULE, tiles), tiles["frames"], 0), e["stop"])
    # the statistics: sums over the rendered tile-frames; the counted form's records are the uncounted form's
    pixel_frames, hits = rendered(e, ad.N_FRAMES)
    assert st["primary_rays"] == pixel_frames and st["primary_hits"] == hits and st["shadow_rays"] == hits * ac.BUNNY_LIGHT_SAMPLES
    assert st["kernel_ms"] > 0 and pixel_frames < ad.N_FRAMES * view.nx * view.ny
    rgb2, shade2 = bunny.render_view_adaptive(view, ac.SEEDS, ad.RULE, ac.N_PAIRS, want_shade=True)
    assert shade2.tobytes() == shade.tobytes() and np.array_equal(rgb2, rgb)
    assert np.array_equal(bunny.render_view_adaptive(view, ac.SEEDS, ad.RULE, ac.N_PAIRS), e["rgb8"])          # rgb alone
    for offset in ((1,) if fixture == "bunny" else range(4)):
        d_rgb, d_shade, d_tiles, d_mom, _ = adaptive_on_device(rtx, torch, bunny, view, ac.SEEDS, ad.RULE, rgb_offset=offset)
        check_adaptive(d_rgb, d_shade, d_tiles, e, "%s, device variant, offset %d" % (fixture, offset))
        assert ad.same_moments(d_mom, e["mom"])


def test_the_yards_adaptive_mean_unposed_and_posed(rtx, torch, orc):
    view = ac.yard_view(rtx)
    seeds = ac.SEEDS[:ac.YARD_FRAMES]
    with rs.open_yard(rtx, ac.table(orc, 3)) as scene:
        with pytest.raises(rtx.RtxError) as refused:                     # a posed call on a device without a pose
            scene.render_view_adaptive(view, seeds, ad.YARD_RULE, ac.N_PAIRS, posed=True)
        assert refused.value.code == rtx.ERR_BAD_ARG
        scene.pose_prims(**pm.given(rtx, ac.YARD_POSE[1]))
        for fixture, posed in (("yard", False), ("yard_posed", True), ("yard", False)):
            e = ad.expected(orc, rtx, fixture)
            rgb, shade, tiles, st = scene.render_view_adaptive(view, seeds, ad.YARD_RULE, ac.N_PAIRS, posed=posed, want_shade=True,
                                                               want_tiles=True, stats=True)
            check_adaptive(rgb, shade, tiles, e, fixture + ", host variant")
            assert st["primary_rays"] == int(e["mom"]["frames"].sum()) * pm.NB_RAY
            d_rgb, d_shade, d_tiles, d_mom, _ = adaptive_on_device(rtx, torch, scene, view, seeds, ad.YARD_RULE, rgb_offset=2, posed=posed)
            check_adaptive(d_rgb, d_shade, d_tiles, e, fixture + ", device variant")
            assert ad.same_moments(d_mom, e["mom"])


def test_a_given_light(rtx, torch, orc, bunny):
    """another light with a count of seven, against the oracle's frames under it through the numpy statements; then the
    scene's own light, given: the unlit fixture again"""
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
    errs = np.array([h["err"] for h in e["history"]]).astype(np.float64)
    assert (e["stop"] == 0).any() and (e["stop"] > 2).any() and (np.abs(errs - rule[1]) / rule[1]).min() >= 0.01
    light = rtx.Scene.make_light(tri, count)
    view = bunny.own_view()
    rgb, shade, tiles, st = bunny.render_view_adaptive(view, ac.SEEDS[:4], rule, ac.N_PAIRS, light=light, want_shade=True, want_tiles=True,
                                                       stats=True)
    check_adaptive(rgb, shade, tiles, e, "far_side x 7, host variant")
    assert st["shadow_rays"] == 7 * st["primary_hits"]
    d_rgb, d_shade, d_tiles, d_mom, _ = adaptive_on_device(rtx, torch, bunny, view, ac.SEEDS[:4], rule, light=light)
    check_adaptive(d_rgb, d_shade, d_tiles, e, "far_side x 7, device variant")
    own = bunny.light()
    own.nb_light_sample = 0
    rgb, shade, tiles = bunny.render_view_adaptive(view, ac.SEEDS, ad.RULE, ac.N_PAIRS, light=own, want_shade=True, want_tiles=True)
    check_adaptive(rgb, shade, tiles, ad.expected(orc, rtx, "bunny"), "the scene's own light, given")


# ---------------------------------------------------------------------------------------------- 3: the equivalences
@pytest.mark.parametrize("n", (1, 3, 8))
def test_a_rule_that_never_stops_is_the_mean(rtx, torch, bunny, n):
    """min_frames = n_frames: outputs and the sum / hit_frames words equal rtx_render_view_mean's"""
    view = bunny.own_view()
    w, h = ac.BUNNY_FRAME
    d_acc, m_shade, m_rgb = Guarded(torch, 16 * w * h), Guarded(torch, 16 * w * h), Guarded(torch, 3 * w * h, 1)
    bunny.render_view_mean_device(0, view, ac.SEEDS[:n], ac.N_PAIRS, d_acc.ptr, m_rgb.ptr, m_shade.ptr, stream_of(torch))
    d_rgb, d_shade, d_tiles, d_mom, _ = adaptive_on_device(rtx, torch, bunny, view, ac.SEEDS[:n], (n, 0.0))
    acc = d_acc.get(rtx.ACCUM_PIXEL_DTYPE).reshape(h, w)
    assert np.array_equal(bits(d_mom["sum"]), bits(acc["sum"])) and np.array_equal(d_mom["hit_frames"], acc["hit_frames"])
    assert (d_mom["frames"] == n).all() and (d_tiles["frames"] == n).all()
    assert d_shade.tobytes() == m_shade.get(rtx.PIXEL_SHADE_DTYPE).reshape(h, w).tobytes()
    assert np.array_equal(d_rgb, m_rgb.get().reshape(h, w, 3))
    rgb, shade = bunny.render_view_adaptive(view, ac.SEEDS[:n], (n, INF), ac.N_PAIRS, want_shade=True)
    m = bunny.render_view_mean(view, ac.SEEDS[:n], ac.N_PAIRS, want_shade=True)
    assert shade.tobytes() == m[1].tobytes() and np.array_equal(rgb, m[0])


def test_min_frames_of_one_is_the_one_frame_mean(rtx, torch, bunny):
    """the trap the header names: after one frame the variance is exactly 0, so every tile stops for any threshold"""
    view = bunny.own_view()
    m_rgb, m_shade = bunny.render_view_mean(view, ac.SEEDS[:1], ac.N_PAIRS, want_shade=True)
    for max_variance in (0.0, INF):
        rgb, shade, tiles = bunny.render_view_adaptive(view, ac.SEEDS[:5], (1, max_variance), ac.N_PAIRS, want_shade=True, want_tiles=True)
        assert shade.tobytes() == m_shade.tobytes() and np.array_equal(rgb, m_rgb)
        assert (tiles["frames"] == 1).all() and (bits(tiles["err"]) == 0).all()


# ---------------------------------------------------------------------------------------------- 4: continue
def test_three_and_five_frames_are_eight(rtx, torch, orc, bunny):
    view = bunny.own_view()
    e = ad.expected(orc, rtx, "bunny")
    *_, state = adaptive_on_device(rtx, torch, bunny, view, ac.SEEDS[:3], ad.RULE)
    three = ad.expected(orc, rtx, "bunny", 3)
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
    print("tiles resumed under the stricter rule:\n%s" % resumed.astype(int))
    assert resumed.sum() >= 2 and still.sum() >= 2                       # the lit ground resumes, the sky (error 0) does not
    e["linear"] = ad.np_divide_own(e["mom"])
    e["rgb8"] = ac.oracle_bytes(orc, e["linear"])
    e["hits"] = np.minimum(e["mom"]["hit_frames"], 255).astype(np.uint8)
    *_, state = adaptive_on_device(rtx, torch, bunny, view, ac.SEEDS[:4], ad.RULE)
    d_rgb, d_shade, d_tiles, d_mom, _ = adaptive_on_device(rtx, torch, bunny, view, ac.SEEDS[4:], strict, state=state)
    check_adaptive(d_rgb, d_shade, d_tiles, e, "4 frames, then 4 under a stricter rule")
    assert ad.same_moments(d_mom, e["mom"])


# ---------------------------------------------------------------------------------------------- 5: state
def test_an_adaptive_call_leaves_the_scene_untouched(rtx, torch, orc):
    with rs.open_yard(rtx, ac.table(orc, 4)) as scene:
        view = scene.own_view()
        mean_view = ac.yard_view(rtx)

        def state():
            return (scene.debug_samples().tobytes(), scene.samples_at().tobytes(), scene.render_rows().tobytes(),
                    scene.render_view_rows(view).tobytes(), scene.render_view(view, want_shade=True)[1].tobytes(),
                    scene.debug_light_points(scene.light()).tobytes(), scene.info(),
                    scene.render_view_mean(mean_view, ac.SEEDS[:3], ac.N_PAIRS, want_shade=True)[1].tobytes())

        before = state()
        scene.render_view_adaptive(mean_view, ac.SEEDS[:3], ad.YARD_RULE, ac.N_PAIRS)
        adaptive_on_device(rtx, torch, scene, mean_view, ac.SEEDS[:3], ad.YARD_RULE, n_pairs=7001, light=rtx.Scene.make_light(*pm.POSE_LIGHT))
        assert state() == before


def test_device_resident_calls_on_a_stream_of_their_own_and_a_host_mean_behind_them(rtx, torch, orc, bunny):
    """device-resident launches on one device are ordered on one stream; the host entry points wait for the most recent of
    them by an event before they reuse the scratch table, the scratch records and the light points"""
    view = bunny.own_view()
    w, h = ac.BUNNY_FRAME
    e8, e3 = ad.expected(orc, rtx, "bunny"), ad.expected(orc, rtx, "bunny", 3)
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    bufs = [adaptive_on_device(rtx, torch, bunny, view, ac.SEEDS[:n], ad.RULE, stream=side.cuda_stream) for n in (8, 3)]
    m_rgb, m_shade = bunny.render_view_mean(view, ac.SEEDS[:7], ac.N_PAIRS, want_shade=True)       # nothing waited for in between
    rgb, shade, tiles = bunny.render_view_adaptive(view, ac.SEEDS, ad.RULE, ac.N_PAIRS, want_shade=True, want_tiles=True)
    side.synchronize()
    m = ac.expected(orc, rtx, "bunny", 7)
    assert np.array_equal(bits(m_shade["linear"]), bits(m["linear"])) and np.array_equal(m_rgb, m["rgb8"])
    check_adaptive(rgb, shade, tiles, e8, "host variant behind two device-resident calls")
    for (d_rgb, d_shade, d_tiles, d_mom), e in zip(bufs, (e8, e3)):
        check_adaptive(d_rgb.get().reshape(h, w, 3), d_shade.get(rtx.PIXEL_SHADE_DTYPE).reshape(h, w),
                       d_tiles.get(rtx.TILE_STATE_DTYPE).reshape(e["stop"].shape), e, "device-resident, side stream")
        assert ad.same_moments(d_mom.get(rtx.MOMENT_PIXEL_DTYPE).reshape(h, w), e["mom"])
