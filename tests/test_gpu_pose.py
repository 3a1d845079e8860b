"""GPU parity of posing (rtx_scene_pose, rtx_scene_pose_device, the posed calls and the pose kernels behind them): the
device's posed records word for word against the host statement, and posed views, ray queries and shaded rays of an
uploaded scene against an ORACLE SCENE CREATED WITH THE POSED VERTICES (tests/pose_sets.py, whose conditions
tests/test_pose_sets.py asserts without a GPU).  Every comparison is for equal bits or bytes."""
import importlib
import os

import numpy as np
import pytest

import light_sets as ls
import pose_sets as ps
import query_sets as qs
import shade_sets as ss
import view_sets as vs
from query_sets import F, H, NO_HIT, W, bits

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUNNY = os.path.join(ROOT, "models", "big_bunny.obj")


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


def lib_view(rtx, v, rect=None):
    return rtx.Scene.view(v[0][0], v[0][1], rect=rect, **vs.camera(v))


def same_records(got, want, what):
    for g, w, part in zip(got, want, ("primitive", "shading", "node")):
        bad = np.argwhere(g != w)
        assert not len(bad), "%s: %s records differ at (record, word) %s" % (what, part, bad[:6].tolist())


# ---------------------------------------------------------------------------------------------- 1: the records
@pytest.mark.parametrize("name", ps.BUNNY_POSES)
def test_device_records_are_the_hosts_on_the_bunny(rtx, orc, samples_seeded, bunny, name):
    torch = pytest.importorskip("torch")
    pose = ps.bunny_pose(orc, name)
    st = bunny.pose(pose, stats=True)
    assert st["kernel_ms"] > 0 and st["rays"] == 0
    same_records(bunny.debug_pose(), bunny.posed_records(pose), name + ", host variant, index ranks")
    rank = np.random.default_rng(3).permutation(4969).astype(np.uint32)
    bunny.pose(pose, tie_rank=rank)
    same_records(bunny.debug_pose(), bunny.posed_records(pose, tie_rank=rank), name + ", host variant, given ranks")
    d_pose, d_rank = torch.from_numpy(pose).to("cuda:0"), torch.from_numpy(rank.view(np.int32)).to("cuda:0")
    torch.cuda.synchronize()
    bunny.pose_device(0, d_pose.data_ptr(), d_rank.data_ptr(), torch.cuda.current_stream().cuda_stream)
    same_records(bunny.debug_pose(), bunny.posed_records(pose, tie_rank=rank), name + ", device variant, given ranks")
    bunny.pose_device(0, d_pose.data_ptr(), None, torch.cuda.current_stream().cuda_stream)
    same_records(bunny.debug_pose(), bunny.posed_records(pose), name + ", device variant, index ranks")
    torch.cuda.synchronize()


def test_device_records_are_the_hosts_on_the_small_scenes(rtx, orc, samples_seeded):
    torch = pytest.importorskip("torch")
    scenes = dict(ps.small_scenes(rtx))
    scenes["bunny_brute"] = (ps.base(orc)[0], None, None, dict(accel=rtx.ACCEL_BRUTE), ps.bunny_pose(orc, "tilt"))
    scenes["soup20000"] = (rtx.synthetic_mesh(20000), None, None, {}, rtx.synthetic_mesh(20000, seed=4242))
    for name, sc in scenes.items():
        with ps.open_small(rtx, samples_seeded, sc) as scene:
            own = np.ascontiguousarray(scene.tris.copy())
            for pose, what in ((own, "identity"), (sc[4], "posed"), (own, "identity again")):
                scene.pose(pose)
                same_records(scene.debug_pose(), scene.posed_records(pose), "%s %s, host variant" % (name, what))
            d_pose = torch.from_numpy(np.ascontiguousarray(sc[4])).to("cuda:0")
            torch.cuda.synchronize()
            scene.pose_device(0, d_pose.data_ptr(), None, torch.cuda.current_stream().cuda_stream)
            same_records(scene.debug_pose(), scene.posed_records(sc[4]), "%s, device variant" % name)
            torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------- 2: posed views
@pytest.mark.parametrize("name", ps.BUNNY_POSES)
def test_posed_view_is_the_oracle_scene_with_the_posed_vertices(rtx, orc, samples_seeded, bunny, name):
    p = ps.posed(orc, samples_seeded, name)
    bunny.pose(p["pose"])
    view = lib_view(rtx, ps.SIDE)
    rgb, shade, hits, st = bunny.render_view(view, stats=True, want_shade=True, want_hits=True, posed=True)
    assert np.array_equal(rgb, p["frame"]), "%s: bytes differ from the oracle scene at (y, x) %s" % (
        name, np.argwhere((rgb != p["frame"]).any(axis=2))[:8].tolist())
    assert np.array_equal(bits(shade["linear"]), bits(p["lin"])), name + ": linear differs from the oracle scene's"
    assert np.array_equal(shade["rgb8"], rgb), name
    assert np.array_equal(hits["prim"][:, :, 0], p["tri"]), name + ": hit primitives differ"
    assert st["primary_hits"] == p["stats"]["primary_hits"] and st["shadow_rays"] == p["stats"]["shadow_rays"], (name, st)
    # the hit records are rtx_trace_rays_posed's, their normals the posed triangles'
    o, d, _, _, _ = ss.camera_raw_rays(orc, ps.SIDE[0][0], ps.SIDE[0][1], ps.SIDE[1], ps.SIDE[2], vs.UP, ps.SIDE[3], samples_seeded, 1)
    traced = bunny.trace_rays(o, d, keep_order=True, posed=True)
    assert hits.reshape(-1).tobytes() == traced.tobytes(), name
    hit = traced["prim"] != NO_HIT
    normals = ps.tables(orc, samples_seeded, name)["normals"]
    assert np.array_equal(bits(traced["normal"][hit]), bits(normals[traced["prim"][hit]])), name
    assert np.array_equal(bunny.render_view(view, posed=True), rgb)                     # out_rgb alone, no stats


def test_posed_view_records_rectangles_and_a_light(rtx, orc, samples_seeded, bunny):
    p = ps.posed(orc, samples_seeded, "turn")
    s = ps.composition(orc, samples_seeded, "turn")
    bunny.pose(p["pose"])
    view = lib_view(rtx, ps.SIDE)
    rgb, shade, hits = bunny.render_view(view, want_shade=True, want_hits=True, posed=True)
    assert shade.reshape(-1).tobytes() == s["shade"].tobytes(), "shade records differ from the composition on the posed oracle scene"
    qs.check_hits(hits.reshape(-1), s["hit"], ps.tables(orc, samples_seeded, "turn")["normals"], "turn: hit records")
    for rect in vs.SIDE_RECTS:
        x0, y0, nx, ny = rect
        got = bunny.render_view(lib_view(rtx, ps.SIDE, rect=rect), want_shade=True, want_hits=True, posed=True)
        assert np.array_equal(got[0], p["frame"][y0:y0 + ny, x0:x0 + nx]), rect
        assert got[1].tobytes() == np.ascontiguousarray(shade[y0:y0 + ny, x0:x0 + nx]).tobytes(), rect
        assert got[2].tobytes() == np.ascontiguousarray(hits[y0:y0 + ny, x0:x0 + nx]).tobytes(), rect
    # under a given light: the oracle scene created with the posed vertices AND that light
    tri, count = ls.SIDE_LIGHTS[ps.POSE_LIGHT]
    light = rtx.Scene.make_light(tri, count)
    frame, ost = ps.lit_frame(orc, samples_seeded, "turn", ps.POSE_LIGHT)
    lit = bunny.render_view(view, stats=True, want_shade=True, posed=True, light=light)
    assert np.array_equal(lit[0], frame), "lit posed view differs from the oracle scene at %s" % np.argwhere((lit[0] != frame).any(axis=2))[:8].tolist()
    assert lit[2]["shadow_rays"] == ost["shadow_rays"] and (lit[0] != rgb).any()
    sl = ps.composition(orc, samples_seeded, "turn", ps.POSE_LIGHT)
    assert lit[1].reshape(-1).tobytes() == sl["shade"].tobytes()
    part = ss.take(sl, np.arange(300, 300 + 77))
    for kw in (dict(keep_order=True), dict(force_regroup=True)):
        assert bunny.shade_rays(part["origins"], part["directions"], posed=True, light=light, **kw).tobytes() == part["shade"].tobytes(), kw


# ---------------------------------------------------------------------------------------------- 3: queries and shading
@pytest.mark.parametrize("name", ["turn", "tilt"])
def test_ray_queries_and_shading_on_the_posed_scene(rtx, orc, samples_seeded, bunny, name):
    (ro, rd, exp), (to, tt, texp, occ) = ps.query_set(orc, samples_seeded, name)
    normals = ps.tables(orc, samples_seeded, name)["normals"]
    bunny.pose(ps.posed(orc, samples_seeded, name)["pose"])
    for n in (1, 63, 64, 65, 127, 129, len(ro)):
        for kw in (dict(keep_order=True), dict(force_regroup=True), dict()):
            qs.check_hits(bunny.trace_rays(ro[:n], rd[:n], posed=True, **kw), exp[:n], normals, "%s trace %d %s" % (name, n, kw))
            got = bunny.occluded_rays(to[:n], tt[:n], posed=True, **kw)
            assert np.array_equal(got, occ[:n]), (name, n, kw, np.nonzero(got != occ[:n])[0][:8])
    got, st = bunny.trace_rays(ro, rd, posed=True, stats=True)
    assert st["primary_rays"] == len(ro) and st["primary_hits"] == int((exp["prim"] != NO_HIT).sum())
    # shading: the composition on the posed oracle scene, in the caller's order and regrouped, sizes around a wavefront
    s = ps.composition(orc, samples_seeded, name) if name == "turn" else None
    if s is not None:
        for n0, n in ((0, 64), (100, 65), (200, 127), (500, 1)):
            part = ss.take(s, np.arange(n0, n0 + n))
            for kw in (dict(keep_order=True), dict(force_regroup=True)):
                shade, hits = bunny.shade_rays(part["origins"], part["directions"], want_hits=True, posed=True, **kw)
                assert shade.tobytes() == part["shade"].tobytes(), (n0, n, kw)
                assert hits.tobytes() == bunny.trace_rays(part["origins"], part["directions"], keep_order=True, posed=True).tobytes()


# ---------------------------------------------------------------------------------------------- 4: hard rays and ties
def test_hard_rays_follow_the_reference_tree_rule(rtx, orc, samples_seeded, bunny):
    o, d, exp, twin = ps.hard_rays(orc, samples_seeded, "turn")
    pose = ps.posed(orc, samples_seeded, "turn")["pose"]
    normals = ps.tables(orc, samples_seeded, "turn")["normals"]
    bunny.pose(pose, reference_tree=rtx.REFTREE_ALWAYS)
    for kw in (dict(keep_order=True), dict(force_regroup=True)):
        qs.check_hits(bunny.trace_rays(o, d, posed=True, **kw), exp, normals, "hard rays under RTX_REFTREE_ALWAYS %s" % kw)
    # ordinary rays do not depend on the tree
    (ro, rd, qexp), _ = ps.query_set(orc, samples_seeded, "turn")
    qs.check_hits(bunny.trace_rays(ro, rd, posed=True), qexp, normals, "ordinary rays under RTX_REFTREE_ALWAYS")
    # RTX_REFTREE_NEVER: the refitted stream with the reference's box test — some tree over these primitives; it terminates,
    # and every hit it reports is the twin's or a miss
    bunny.pose(pose, reference_tree=rtx.REFTREE_NEVER)
    got = bunny.trace_rays(o, d, posed=True, keep_order=True)
    hit = got["prim"] != NO_HIT
    assert np.array_equal(got["prim"][hit], twin["prim"][hit])


def test_ties_between_coincident_posed_triangles(rtx, orc, samples_seeded):
    o, d = ps.TIE_RAYS
    rgb = np.ones((3, 3), F)
    osc = orc.Scene(8, 8, ps.TIE_POSE, rgb, samples_seeded, **ps.TIE_KW)
    exp, _ = qs.oracle_hits(orc, osc, o, d, qs.HIT_DTYPE)
    assert exp["prim"][0] in (0, 1) and exp["t"][0] > 1
    with rtx.Scene(8, 8, ps.TIE_TRIS, rgb, samples_seeded[:4096], **ps.TIE_KW) as scene:
        assert scene.trace_rays(o, d)["prim"][0] == 0                          # unposed: the nearer one
        scene.pose(ps.TIE_POSE, reference_tree=rtx.REFTREE_ALWAYS)
        got = scene.trace_rays(o, d, posed=True)
        assert np.array_equal(got["prim"], exp["prim"]) and np.array_equal(bits(got["t"]), bits(exp["t"]))
        scene.pose(ps.TIE_POSE, reference_tree=rtx.REFTREE_NEVER)
        assert scene.trace_rays(o, d, posed=True)["prim"][0] == 1              # NULL ranks: the larger index
        scene.pose(ps.TIE_POSE, tie_rank=np.array([5, 3, 0], np.uint32), reference_tree=rtx.REFTREE_NEVER)
        assert scene.trace_rays(o, d, posed=True)["prim"][0] == 0              # the larger tie_rank
        scene.pose(ps.TIE_POSE, tie_rank=np.array([2, 3, 9], np.uint32), reference_tree=rtx.REFTREE_ALWAYS)
        assert scene.trace_rays(o, d, posed=True)["prim"][0] == 1              # given ranks go before the tree's
        assert scene.trace_rays(o, d)["prim"][0] == 0
    osc.close()


# ---------------------------------------------------------------------------------------------- 5: identity, state
def usual(rtx, scene, orc, samples, **kw):
    (ro, rd, _), (to, tt, _, _) = ps.query_set(orc, samples, "identity")
    view = lib_view(rtx, ps.SIDE)
    v = scene.render_view(view, want_shade=True, want_hits=True, **kw)
    sh = scene.shade_rays(ro[:130], rd[:130], want_hits=True, force_regroup=True, **kw)
    return [x.tobytes() for x in v] + [x.tobytes() for x in sh] + [scene.trace_rays(ro, rd, **kw).tobytes(),
                                                                   scene.occluded_rays(to, tt, **kw).tobytes()]


def test_identity_posed_calls_are_their_unposed_twins(rtx, orc, samples_seeded, bunny):
    plain = usual(rtx, bunny, orc, samples_seeded)
    bunny.pose(ps.bunny_pose(orc, "identity"), reference_tree=rtx.REFTREE_AUTO)       # the scene's own rule: its own tree's ranks
    assert usual(rtx, bunny, orc, samples_seeded, posed=True) == plain
    light = rtx.Scene.make_light(*ls.SIDE_LIGHTS[ps.POSE_LIGHT])
    view = lib_view(rtx, ps.SIDE)
    assert bunny.render_view(view, want_shade=True, posed=True, light=light)[1].tobytes() == \
        bunny.render_view(view, want_shade=True, light=light)[1].tobytes()


def test_state(rtx, orc, samples_seeded):
    view = lib_view(rtx, ps.SIDE)
    frames = {n: ps.posed(orc, samples_seeded, n)["frame"] for n in ("identity", "turn", "shift")}
    with rtx.default_scene([BUNNY], W, H, samples_seeded) as scene, rtx.default_scene([BUNNY], W, H, samples_seeded) as other:
        # a posed call before any pose
        with pytest.raises(rtx.RtxError) as e:
            scene.render_view(view, posed=True)
        assert e.value.code == rtx.ERR_BAD_ARG
        with pytest.raises(rtx.RtxError) as e:
            scene.debug_pose()
        assert e.value.code == rtx.ERR_BAD_ARG
        before = usual(rtx, scene, orc, samples_seeded) + [scene.render_rows().tobytes(), scene.render_view_rows(view).tobytes()]
        with pytest.raises(rtx.RtxError) as e:                                         # (the upload alone makes no pose)
            scene.trace_rays(np.zeros((1, 3), F), np.ones((1, 3), F), posed=True)
        assert e.value.code == rtx.ERR_BAD_ARG
        # turn, then shift, then identity: each its own frame, nothing left over
        for name in ("turn", "shift", "identity", "turn"):
            scene.pose(ps.bunny_pose(orc, name))
            assert np.array_equal(scene.render_view(view, posed=True), frames[name]), name
            assert np.array_equal(scene.render_view(view), frames["identity"]), name + ": the unposed view changed"
        # two live scenes, each its own pose
        other.pose(ps.bunny_pose(orc, "shift"))
        assert np.array_equal(scene.render_view(view, posed=True), frames["turn"])
        assert np.array_equal(other.render_view(view, posed=True), frames["shift"])
        # unposed calls after a pose: equal bytes through every path
        after = usual(rtx, scene, orc, samples_seeded) + [scene.render_rows().tobytes(), scene.render_view_rows(view).tobytes()]
        assert after == before
        with pytest.raises(rtx.RtxError) as e:
            bad = ps.bunny_pose(orc, "turn").copy()
            bad[7, 2] = 10000.5
            scene.pose(bad)
        assert e.value.code == rtx.ERR_UNSUPPORTED
        assert np.array_equal(scene.render_view(view, posed=True), frames["turn"])     # a refused pose changes nothing


def test_spheres_and_two_rays_per_pixel(rtx, orc, samples_seeded):
    fx = vs.soup_view(orc, samples_seeded)
    a = fx["a"]
    _, _, tris, rgb, _ = a["args"]
    rng = np.random.default_rng(5)
    # every triangle drawn towards the origin by 3 % and moved by up to 0.3: within the scene's largest coordinate
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
        same_records(scene.debug_pose(), scene.posed_records(pose, tie_rank=scene.debug_pose()[1][:, 3].copy()), "soup with spheres")
        got, gst = scene.render_view(view, stats=True, posed=True)
        assert np.array_equal(got, frame), np.argwhere((got != frame).any(axis=2))[:8].tolist()
        assert gst["primary_hits"] == st["primary_hits"]
        assert np.array_equal(scene.render_view(view), fx["frame"])
        scene.pose(tris)
        assert np.array_equal(scene.render_view(view, posed=True), fx["frame"])


# ---------------------------------------------------------------------------------------------- 6: device-resident
def test_device_resident_pose_and_two_posed_views_on_one_stream(rtx, orc, samples_seeded, bunny):
    torch = pytest.importorskip("torch")
    assert torch.cuda.is_available(), "torch sees no GPU"
    turn, shift = (ps.posed(orc, samples_seeded, n) for n in ("turn", "shift"))
    view = lib_view(rtx, ps.SIDE)
    n = view.nx * view.ny
    stream = torch.cuda.Stream(device="cuda:0")
    with torch.cuda.stream(stream):
        d_turn, d_shift = (torch.from_numpy(p["pose"].copy()).to("cuda:0") for p in (turn, shift))
        bufs = [[torch.full((size + 16,), 0xAA, dtype=torch.uint8, device="cuda:0") for size in (n * 3, n * 16, n * 32)] for _ in range(2)]
        stream.synchronize()
        # pose, view, view under a light, a second pose and its view: one stream, nothing waited for between
        bunny.pose_device(0, d_turn.data_ptr(), None, stream.cuda_stream)
        bunny.render_view_device(0, view, bufs[0][0].data_ptr(), bufs[0][1].data_ptr(), bufs[0][2].data_ptr(), stream.cuda_stream, posed=True)
        light = rtx.Scene.make_light(*ls.SIDE_LIGHTS[ps.POSE_LIGHT])
        lit = torch.full((n * 3,), 0xAA, dtype=torch.uint8, device="cuda:0")
        bunny.render_view_device(0, view, lit.data_ptr(), None, None, stream.cuda_stream, posed=True, light=light)
        bunny.pose_device(0, d_shift.data_ptr(), None, stream.cuda_stream)
        bunny.render_view_device(0, view, bufs[1][0].data_ptr(), bufs[1][1].data_ptr(), bufs[1][2].data_ptr(), stream.cuda_stream, posed=True)
        # ... and a host posed call right behind them, on the library's stream: it waits for the event
        host = bunny.render_view(view, posed=True)
        assert np.array_equal(host, shift["frame"])
        stream.synchronize()
        for p, b in zip((turn, shift), bufs):
            rgb, shade, hits = (t.cpu().numpy() for t in b)
            assert rgb[:n * 3].tobytes() == p["frame"].tobytes() and (rgb[n * 3:] == 0xAA).all()
            assert np.array_equal(bits(shade[:n * 16].view(rtx.rtx.PIXEL_SHADE_DTYPE)["linear"]), bits(p["lin"].reshape(-1, 3)))
            assert (shade[n * 16:] == 0xAA).all()
            assert np.array_equal(hits[:n * 32].view(rtx.rtx.RAY_HIT_DTYPE)["prim"], p["tri"].reshape(-1)) and (hits[n * 32:] == 0xAA).all()
        assert lit.cpu().numpy().tobytes() == ps.lit_frame(orc, samples_seeded, "turn", ps.POSE_LIGHT)[0].tobytes()
        # the ray-batch device forms against the posed oracle scene (the device holds `shift`)
        (ro, rd, exp), (to, tt, _, occ) = ps.query_set(orc, samples_seeded, "shift")
        m = len(ro)
        d_o, d_d, d_to, d_tt = (torch.from_numpy(np.ascontiguousarray(x)).to("cuda:0") for x in (ro, rd, to, tt))
        d_hits = torch.zeros(m * 32, dtype=torch.uint8, device="cuda:0")
        d_occ = torch.zeros(m, dtype=torch.uint8, device="cuda:0")
        d_shade = torch.zeros(m * 16, dtype=torch.uint8, device="cuda:0")
        stream.synchronize()
        bunny.trace_rays_device(0, m, d_o.data_ptr(), d_d.data_ptr(), d_hits.data_ptr(), stream.cuda_stream, force_regroup=True, posed=True)
        bunny.occluded_rays_device(0, m, d_to.data_ptr(), d_tt.data_ptr(), d_occ.data_ptr(), stream.cuda_stream, posed=True)
        bunny.shade_rays_device(0, m, d_o.data_ptr(), d_d.data_ptr(), d_shade.data_ptr(), None, stream.cuda_stream, posed=True)
        stream.synchronize()
        qs.check_hits(d_hits.cpu().numpy().view(rtx.rtx.RAY_HIT_DTYPE), exp, None, "rtx_trace_rays_posed_device")
        assert np.array_equal(d_occ.cpu().numpy(), occ)
        assert d_shade.cpu().numpy().tobytes() == bunny.shade_rays(ro, rd, posed=True).tobytes()


# ---------------------------------------------------------------------------------------------- 7: a turntable
def test_four_turns_of_the_mesh(rtx, orc, samples_seeded, bunny):
    view = lib_view(rtx, ps.TURNTABLE_VIEW)
    for deg, (pose, frame) in zip(ps.TURNTABLE_DEGREES, ps.turntable(orc, samples_seeded)):
        bunny.pose(pose)
        got = bunny.render_view(view, posed=True)
        assert got.shape == (16, 24, 3)
        assert np.array_equal(got, frame), "turn %g: differs at %s" % (deg, np.argwhere((got != frame).any(axis=2))[:8].tolist())
