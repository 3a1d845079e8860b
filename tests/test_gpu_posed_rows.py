"""GPU parity of rtx_render_view_rows_posed (and its device-resident variant): a pose of an uploaded scene through the
render pipeline.  The device's plane records and posed aimed stream word for word against the host statement; posed
pipeline frames against ORACLE SCENES CREATED WITH THE POSED VERTICES (tests/pose_sets.py, tests/posed_rows_sets.py, whose
conditions tests/test_pose_sets.py and tests/test_posed_rows_sets.py assert without a GPU) and against
rtx_render_view_posed; the aim cache, the pose's ordering rule and the state a posed call leaves.  Every comparison is for
equal words or bytes."""
import ctypes as C
import importlib
import os

import numpy as np
import pytest

import light_sets as ls
import lit_rows_sets as lr
import pose_sets as ps
import posed_rows_sets as pr
import sequence_sets as sq
import view_sets as vs
from query_sets import F, H, W

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUNNY = os.path.join(ROOT, "models", "big_bunny.obj")
GUARD = 0xA5


@pytest.fixture(scope="module")
def rtx():
    mod = importlib.import_module("ray-tracer-rust_amd")
    assert mod.device_count() >= 1, "no HIP device: the product path has no CPU fallback"
    return mod


@pytest.fixture(scope="module")
def bunny(rtx, orc, samples_seeded):
    """big_bunny + ground created 32 x 32 with the default camera: the scene every bunny pose is applied to"""
    scene = rtx.default_scene([BUNNY], W, H, samples_seeded)
    assert scene.info()["n_tris"] == 4969 and scene.info()["n_global"] == 1 and scene.pose_bound() == F(ps.M)
    yield scene
    scene.close()


def lib_view(rtx, v, rows=None):
    (w, h) = v[0]
    return rtx.Scene.view(w, h, rect=None if rows is None else (0, rows[0], w, rows[1]), **vs.camera(v))


def where(got, want):
    return np.argwhere((got != want).any(axis=2))[:8].tolist()


# ---------------------------------------------------------------------------------------------- 1: planes and aimed stream
@pytest.mark.parametrize("name", ["tilt", "turn", "lifted", "soup257_ground", "soup256", "soup255_brute"])
def test_device_planes_and_aimed_stream_are_the_hosts(rtx, orc, samples_seeded, name):
    torch = pytest.importorskip("torch")
    open_scene, pose, eyes = pr.record_cases(rtx, orc, samples_seeded)[name]

    def same(scene, p, what):
        for eye in eyes:
            want_planes, want_aimed = scene.posed_pipeline_records(p, eye=eye)
            got_planes = np.full_like(want_planes, 0xA5A5A5A5) if len(want_planes) else want_planes.copy()
            got_aimed = np.zeros_like(want_aimed)
            rc = rtx.rtx._lib.rtx_debug_pose_pipeline(scene.handle, 0, np.asarray(eye, F).ctypes.data_as(rtx.rtx.f32p),
                                                      got_planes.ctypes.data_as(rtx.rtx.u32p), got_aimed.ctypes.data_as(rtx.rtx.u32p))
            assert rc == rtx.OK, (name, what, rc)
            bad = np.argwhere(got_planes != want_planes)
            assert not len(bad), "%s %s: plane records differ at (record, word) %s: %s / %s" % (
                name, what, bad[:6].tolist(), got_planes[bad[0][0]].tolist(), want_planes[bad[0][0]].tolist())
            bad = np.argwhere(got_aimed != want_aimed)
            assert not len(bad), "%s %s, eye %s: aimed records differ at (record, word) %s" % (name, what, eye, bad[:6].tolist())
        assert np.array_equal(scene.debug_pose_pipeline()[0], want_planes)                  # the planes alone, no eye

    with open_scene() as scene:
        n_global, aims = scene.info()["n_global"], bool(scene.primary_nodes()[1])
        own = np.ascontiguousarray(scene.tris.copy())
        for p, what in ((pose, "posed"), (own, "identity"), (pose, "posed again")):
            scene.pose(p)
            same(scene, p, what + ", rtx_scene_pose")
        d_pose, d_own = (torch.from_numpy(np.ascontiguousarray(x)).to("cuda:0") for x in (pose, own))
        torch.cuda.synchronize()
        stream = torch.cuda.current_stream().cuda_stream
        scene.pose_device(0, d_own.data_ptr(), None, stream)
        scene.pose_device(0, d_pose.data_ptr(), None, stream)
        same(scene, pose, "rtx_scene_pose_device")
        torch.cuda.synchronize()
        if not n_global:                                   # no global triangle: no kernel, nothing written (the guard words stand)
            assert scene.posed_pipeline_records(pose)[0].shape == (0, 16)
        if not aims:                                       # a scene that aims nothing: the pose's own node stream
            assert np.array_equal(scene.debug_pose_pipeline(eye=eyes[0])[1], scene.debug_pose()[2])
        if name == "lifted":                               # level grounds: W components of 0 went up to the smallest subnormal
            assert (scene.debug_pose_pipeline()[0][0][[6, 8]] == 1).all()


# ---------------------------------------------------------------------------------------------- 2: posed frames
@pytest.mark.parametrize("name", ps.BUNNY_POSES)
def test_posed_rows_are_the_oracle_scene_with_the_posed_vertices(rtx, orc, samples_seeded, bunny, name):
    p = ps.posed(orc, samples_seeded, name)
    bunny.pose(p["pose"])
    view = lib_view(rtx, ps.SIDE)
    rgb, st = bunny.render_view_rows(view, stats=True, posed=True)
    assert rgb.shape == (27, 44, 3)
    assert np.array_equal(rgb, p["frame"]), "%s: bytes differ from the oracle scene at (y, x) %s" % (name, where(rgb, p["frame"]))
    assert np.array_equal(rgb, bunny.render_view(view, posed=True)), name + ": bytes differ from rtx_render_view_posed's"
    assert st["primary_rays"] == 44 * 27 and st["primary_hits"] == p["stats"]["primary_hits"], (name, st)
    assert st["shadow_rays"] == p["stats"]["shadow_rays"] and st["redo_tiles"] == 0 and st["kernel_ms"] > 0, (name, st)
    assert np.array_equal(bunny.render_view_rows(view, posed=True), rgb)                  # no stats, the aimed stream standing


def test_the_lifted_ground_frame(rtx, orc, samples_seeded):
    """stale plane records fail here: they would rule the lifted ground out for the patch's shadow rays"""
    L = pr.lifted(orc, samples_seeded)
    view = lib_view(rtx, pr.LIFT_VIEW)
    with pr.lift_scene(rtx, samples_seeded) as scene:
        assert np.array_equal(scene.render_view_rows(view), L["still"])
        scene.pose(pr.lift_pose())
        rgb, st = scene.render_view_rows(view, stats=True, posed=True)
        assert np.array_equal(rgb, L["frame"]), "bytes differ from the oracle scene at (y, x) %s" % where(rgb, L["frame"])
        assert st["primary_hits"] == L["stats"]["primary_hits"] == L["patch_pixels"] + L["ground_pixels"]
        assert np.array_equal(rgb, scene.render_view(view, posed=True))
        assert np.array_equal(scene.render_view_rows(view), L["still"])                  # the unposed planes still serve the scene
        assert np.array_equal(scene.render_view_rows(view, posed=True), L["frame"])


# ---------------------------------------------------------------------------------------------- 3: a light
def test_posed_rows_under_a_given_light(rtx, orc, samples_seeded, bunny):
    tri, count = ls.SIDE_LIGHTS[ps.POSE_LIGHT]
    light = rtx.Scene.make_light(tri, count)
    view = lib_view(rtx, ps.SIDE)
    plain = ps.posed(orc, samples_seeded, "turn")
    bunny.pose(plain["pose"])
    frame, ost = ps.lit_frame(orc, samples_seeded, "turn", ps.POSE_LIGHT)
    rgb, st = bunny.render_view_rows(view, stats=True, posed=True, light=light)
    assert np.array_equal(rgb, frame), "lit posed rows differ from the oracle scene at %s" % where(rgb, frame)
    assert st["shadow_rays"] == ost["shadow_rays"] and (rgb != plain["frame"]).any()
    assert np.array_equal(rgb, bunny.render_view(view, posed=True, light=light))
    assert np.array_equal(bunny.render_view_rows(view, posed=True), plain["frame"])       # the scene's light afterwards
    assert np.array_equal(bunny.render_view_rows(view, light=light), lr_side_frame(orc, samples_seeded))


def lr_side_frame(orc, samples):
    """the unposed 44 x 27 side view under POSE_LIGHT: the identity pose's lit oracle frame"""
    return ps.lit_frame(orc, samples, "identity", ps.POSE_LIGHT)[0]


# ---------------------------------------------------------------------------------------------- 4: identity
def test_the_identity_pose_is_render_view_rows(rtx, orc, samples_seeded, bunny):
    bunny.pose(ps.bunny_pose(orc, "identity"), reference_tree=rtx.REFTREE_AUTO)          # the scene's own rule
    for v in (ps.SIDE, vs.BUNNY_VIEWS["back"], ps.TURNTABLE_VIEW, lr.SIDE):
        view = lib_view(rtx, v)
        want, wst = bunny.render_view_rows(view, stats=True)
        got, gst = bunny.render_view_rows(view, stats=True, posed=True)
        assert got.tobytes() == want.tobytes(), v
        for k in ("primary_rays", "primary_hits", "shadow_rays", "rays", "redo_tiles"):
            assert gst[k] == wst[k], (k, gst, wst)
    own = bunny.own_view()
    assert bunny.render_view_rows(own, posed=True).tobytes() == bunny.render_rows().tobytes()


# ---------------------------------------------------------------------------------------------- 5: row windows
def test_row_windows_off_the_tile_grid(rtx, orc, samples_seeded, bunny):
    p = ps.posed(orc, samples_seeded, "squash")
    bunny.pose(p["pose"])
    (w, h) = ps.SIDE[0]
    assert (w % 8, h % 8) == (4, 3)
    for y0, ny in ((3, 13), (8, 8), (h - 1, 1), (0, h), (5, 17)):
        n = ny * w * 3
        buf = np.full(64 + n + 64, GUARD, np.uint8)
        v = lib_view(rtx, ps.SIDE, (y0, ny))
        rc = rtx.rtx._lib.rtx_render_view_rows_posed(bunny.handle, 0, C.byref(v), None, buf[64:].ctypes.data, None)
        assert rc == rtx.OK, (y0, ny)
        assert (buf[:64] == GUARD).all() and (buf[64 + n:] == GUARD).all(), "bytes changed around the output"
        assert np.array_equal(buf[64:64 + n].reshape(ny, w, 3), p["frame"][y0:y0 + ny]), (y0, ny)


# ---------------------------------------------------------------------------------------------- 6: hard rays and the tie
@pytest.mark.parametrize("rule", ["REFTREE_NEVER", "REFTREE_ALWAYS"])
def test_hard_rays_and_the_exact_tie_follow_the_poses_rule(rtx, orc, samples_seeded, rule):
    """P of sequence_sets through its own axis camera: -0.0 direction components on the centre row and column, and an exact
    tie; the frame of rtx_render_view_posed under the same rule, and under RTX_REFTREE_ALWAYS with the scene's own
    triangles the oracle's"""
    hs = vs.hard_scene("P", orc, samples_seeded, rtx)
    hard_tiles, _ = vs.neg_zero_tiles(hs["ref"])
    assert hard_tiles > 0 and hs["ref"]["ties"] > 0
    with rtx.Scene(*hs["args"], **hs["kw"]) as scene:
        v = lib_view(rtx, hs["v"])
        own = np.ascontiguousarray(scene.tris.copy())
        half = np.ascontiguousarray((own * F(0.5)).astype(F))             # exact: coincident triangles stay coincident
        frames = []
        for pose in (own, half):
            scene.pose(pose, reference_tree=getattr(rtx, rule))
            rgb, st = scene.render_view_rows(v, stats=True, posed=True)
            want = scene.render_view(v, posed=True)
            assert np.array_equal(rgb, want), "%s: differs from rtx_render_view_posed at %s" % (rule, where(rgb, want))
            assert st["redo_tiles"] > 0                       # the hard tiles go through the pipeline's reference re-render
            frames.append(rgb)
        assert (frames[0] != frames[1]).any()
        if rule == "REFTREE_ALWAYS":
            assert np.array_equal(frames[0], hs["ref"]["frame"])
        assert np.array_equal(scene.render_view_rows(v), hs["ref"]["frame"])


# ---------------------------------------------------------------------------------------------- 7: spheres, two rays per pixel
def test_spheres_and_two_rays_per_pixel(rtx, orc, samples_seeded):
    fx = vs.soup_view(orc, samples_seeded)
    a = fx["a"]
    _, _, tris, rgb, _ = a["args"]
    rng = np.random.default_rng(5)
    pose = np.ascontiguousarray((0.97 * tris.reshape(-1, 3, 3) + rng.uniform(-0.3, 0.3, size=(len(tris), 1, 3))).reshape(-1, 9).astype(F))
    kw = dict(a["kw"], **vs.camera(vs.SOUP_VIEW))
    osc = orc.Scene(vs.SOUP_VIEW[0][0], vs.SOUP_VIEW[0][1], pose, rgb, samples_seeded, nb_ray=2, **kw)
    frame, st = osc.render_rows(mode=orc.MODE_BVH)
    osc.close()
    assert (frame != fx["frame"]).any(axis=2).sum() >= 20
    with rtx.Scene(*a["args"], nb_ray=2, **a["kw"]) as scene:
        assert np.abs(pose).max() <= scene.pose_bound()
        view = lib_view(rtx, vs.SOUP_VIEW)
        scene.pose(pose, reference_tree=rtx.REFTREE_ALWAYS)
        got, gst = scene.render_view_rows(view, stats=True, posed=True)
        assert np.array_equal(got, frame), where(got, frame)
        assert gst["primary_rays"] == 2 * fx["w"] * fx["h"] and gst["primary_hits"] == st["primary_hits"]
        assert np.array_equal(got, scene.render_view(view, posed=True))
        assert np.array_equal(scene.render_view_rows(view), fx["frame"])


# ---------------------------------------------------------------------------------------------- 8: tile descriptors
def test_a_posed_launch_cuts_tiles_and_finishes_tiles(rtx, orc, samples_seeded, bunny):
    p = ps.posed(orc, samples_seeded, "shift")
    bunny.pose(p["pose"])
    view = lib_view(rtx, ps.SIDE)
    before = len(bunny.launch_timings()[0])
    assert np.array_equal(bunny.render_view_rows(view, posed=True), p["frame"])
    (w, h) = ps.SIDE[0]
    descs = bunny.tile_descs()
    assert len(descs) == sq.launch_tiles(w, h)[1]
    finished, cut = lr.tile_classes(descs, w, h)
    print("posed `shift`, 44 x 27: %d tiles finished by the scheduling pass, %d with a cut, of %d" % (finished, cut, sq.launch_tiles(w, h)[0]))
    assert finished > 0 and cut > 0
    sched, shade = bunny.launch_timings()
    assert len(sched) == min(before + 1, 64) and sched[-1] > 0 and shade[-1] > 0


# ---------------------------------------------------------------------------------------------- 9: state
def test_state(rtx, orc, samples_seeded):
    view, back = lib_view(rtx, ps.SIDE), lib_view(rtx, vs.BUNNY_VIEWS["back"])
    frames = {n: ps.posed(orc, samples_seeded, n)["frame"] for n in ("identity", "turn", "shift")}
    with rtx.default_scene([BUNNY], W, H, samples_seeded) as scene, rtx.default_scene([BUNNY], W, H, samples_seeded) as other:
        usual = scene.render_rows().tobytes()
        # no pose: RTX_ERR_BAD_ARG, through both entry points, and from the diagnostic
        for call in (lambda: scene.render_view_rows(view, posed=True), lambda: scene.debug_pose_pipeline(eye=ps.SIDE[1]),
                     lambda: scene.render_view_rows_device(0, view, 256, 1 << 30, posed=True)):
            with pytest.raises(rtx.RtxError) as e:
                call()
            assert e.value.code == rtx.ERR_BAD_ARG
        back_unposed = scene.render_view_rows(back)
        # posed, unposed, posed rows of ONE eye on one stream: each its own bytes (a shared aim cache would hand one the other's stream)
        scene.pose(ps.bunny_pose(orc, "shift"))
        for k in range(2):
            assert np.array_equal(scene.render_view_rows(view, posed=True), frames["shift"]), k
            assert np.array_equal(scene.render_view_rows(view), frames["identity"]), k
        # ... and the device's two aimed streams are each their own host statement's
        assert np.array_equal(scene.debug_pose_pipeline(eye=ps.SIDE[1])[1],
                              scene.posed_pipeline_records(ps.bunny_pose(orc, "shift"), eye=ps.SIDE[1])[1])
        assert np.array_equal(scene.debug_aimed_nodes(ps.SIDE[1]), scene.aimed_nodes(ps.SIDE[1]))
        assert np.array_equal(scene.render_view_rows(view, posed=True), frames["shift"])
        # a new pose followed by the same eye: the new pose's bytes
        scene.pose(ps.bunny_pose(orc, "turn"))
        assert np.array_equal(scene.render_view_rows(view, posed=True), frames["turn"])
        assert np.array_equal(scene.render_view_rows(back), back_unposed)
        assert np.array_equal(scene.render_view_rows(view, posed=True), frames["turn"])    # another eye in between, unposed
        # a refused pose leaves the previous one rendering
        with pytest.raises(rtx.RtxError) as e:
            bad = ps.bunny_pose(orc, "shift").copy()
            bad[7, 2] = 10000.5
            scene.pose(bad)
        assert e.value.code == rtx.ERR_UNSUPPORTED
        assert np.array_equal(scene.render_view_rows(view, posed=True), frames["turn"])
        # two live scenes, each its own pose
        other.pose(ps.bunny_pose(orc, "shift"))
        for k in range(2):
            assert np.array_equal(scene.render_view_rows(view, posed=True), frames["turn"])
            assert np.array_equal(other.render_view_rows(view, posed=True), frames["shift"])
        assert np.array_equal(other.render_view_rows(view), frames["identity"])
        # the scene's usual bytes afterwards
        assert scene.render_rows().tobytes() == usual and other.render_rows().tobytes() == usual
        assert np.array_equal(scene.render_view(view), frames["identity"])


# ---------------------------------------------------------------------------------------------- 10: device-resident
def test_device_resident_pose_and_two_posed_launches_on_one_stream(rtx, orc, samples_seeded, bunny):
    torch = pytest.importorskip("torch")
    assert torch.cuda.is_available(), "torch sees no GPU"
    turn, shift = (ps.posed(orc, samples_seeded, n) for n in ("turn", "shift"))
    view = lib_view(rtx, ps.SIDE)
    n = view.ny * view.width * 3
    stream = torch.cuda.Stream(device="cuda:0")
    assert stream.cuda_stream != torch.cuda.default_stream().cuda_stream
    with torch.cuda.stream(stream):
        d_turn, d_shift = (torch.from_numpy(p["pose"].copy()).to("cuda:0") for p in (turn, shift))
        bufs = [torch.full((n + 16,), 0xAA, dtype=torch.uint8, device="cuda:0") for _ in range(3)]
        counters = torch.zeros(8, dtype=torch.int64, device="cuda:0")
        stream.synchronize()
        with pytest.raises(rtx.RtxError) as e:
            bunny.render_view_rows_device(0, view, bufs[0].data_ptr(), n - 1, stream.cuda_stream, posed=True)
        assert e.value.code == rtx.ERR_BAD_ARG
        # pose, posed rows, a second pose, its rows twice (the second finds its eye aimed): one stream, one counter block,
        # nothing waited for between
        bunny.pose_device(0, d_turn.data_ptr(), None, stream.cuda_stream)
        bunny.render_view_rows_device(0, view, bufs[0].data_ptr(), bufs[0].numel(), stream.cuda_stream, counters.data_ptr(), posed=True)
        bunny.pose_device(0, d_shift.data_ptr(), None, stream.cuda_stream)
        bunny.render_view_rows_device(0, view, bufs[1].data_ptr(), bufs[1].numel(), stream.cuda_stream, counters.data_ptr(), posed=True)
        bunny.render_view_rows_device(0, view, bufs[2].data_ptr(), bufs[2].numel(), stream.cuda_stream, posed=True)
        # ... and a host posed call right behind them, on the library's stream: it waits for the event
        host = bunny.render_view_rows(view, posed=True)
        assert np.array_equal(host, shift["frame"])
        stream.synchronize()
        for p, b in zip((turn, shift, shift), bufs):
            out = b.cpu().numpy()
            assert out[:n].tobytes() == p["frame"].tobytes() and (out[n:] == 0xAA).all()
        got = counters.cpu().numpy()
        assert int(got[0]) == turn["stats"]["primary_hits"] + shift["stats"]["primary_hits"], got
    assert np.array_equal(bunny.render_view_rows(view), ps.posed(orc, samples_seeded, "identity")["frame"])


def test_a_host_pose_and_a_host_lit_call_behind_device_resident_posed_lit_rows(rtx, orc, samples_seeded, bunny):
    """the host calls overwrite the pose and the light buffers the launch on the caller's stream still reads: both wait"""
    torch = pytest.importorskip("torch")
    assert torch.cuda.is_available(), "torch sees no GPU"
    turn, shift = (ps.posed(orc, samples_seeded, n) for n in ("turn", "shift"))
    light = rtx.Scene.make_light(*ls.SIDE_LIGHTS[ps.POSE_LIGHT])
    other = ls.side(orc, samples_seeded, "point")
    assert other["v"] == ps.SIDE and ps.POSE_LIGHT != "point"
    view = lib_view(rtx, ps.SIDE)
    n = view.ny * view.width * 3
    stream = torch.cuda.Stream(device="cuda:0")
    assert stream.cuda_stream != torch.cuda.default_stream().cuda_stream
    with torch.cuda.stream(stream):
        d_turn = torch.from_numpy(turn["pose"].copy()).to("cuda:0")
        buf = torch.full((n + 16,), GUARD, dtype=torch.uint8, device="cuda:0")
        stream.synchronize()
        bunny.pose_device(0, d_turn.data_ptr(), None, stream.cuda_stream)
        bunny.render_view_rows_device(0, view, buf.data_ptr(), buf.numel(), stream.cuda_stream, posed=True, light=light)
        # nothing waited for: another pose and another light, on the library's stream
        bunny.pose(shift["pose"])
        host = bunny.render_view_rows(view, light=rtx.Scene.make_light(*ls.SIDE_LIGHTS["point"]))
        stream.synchronize()
        out = buf.cpu().numpy()
        want = ps.lit_frame(orc, samples_seeded, "turn", ps.POSE_LIGHT)[0]
        assert out[:n].tobytes() == want.tobytes() and (out[n:] == GUARD).all()
        assert np.array_equal(host, other["frame"]), "host lit rows differ at %s" % where(host, other["frame"])
    assert np.array_equal(bunny.render_view_rows(view, posed=True), shift["frame"])          # the host pose stands


# ---------------------------------------------------------------------------------------------- 11: a turntable
def test_four_turns_of_the_mesh(rtx, orc, samples_seeded, bunny):
    view = lib_view(rtx, ps.TURNTABLE_VIEW)
    for deg, (pose, frame) in zip(ps.TURNTABLE_DEGREES, ps.turntable(orc, samples_seeded)):
        bunny.pose(pose)
        got = bunny.render_view_rows(view, posed=True)
        assert got.shape == (16, 24, 3)
        assert np.array_equal(got, frame), "turn %g: differs at %s" % (deg, where(got, frame))
