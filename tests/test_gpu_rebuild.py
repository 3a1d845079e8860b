"""GPU parity of a pose whose tree is rebuilt on the device (rtx_scene_pose_rebuilt, rtx_scene_pose_rebuilt_device, the
rebuild kernels, the sort and the refit behind them): the device's permutation, records, node words and aimed stream word
for word against the host statement, and every posed call over the rebuilt pose against an ORACLE SCENE CREATED WITH THE
POSED VERTICES and against the same pose's refitted frame (tests/pose_sets.py, tests/posed_rows_sets.py,
tests/rebuild_sets.py, whose conditions tests/test_rebuild_sets.py asserts without a GPU).  Every comparison is for equal
bits or bytes."""
import ctypes as C
import importlib
import os

import numpy as np
import pytest

import light_sets as ls
import pose_sets as ps
import posed_rows_sets as pr
import query_sets as qs
import rebuild_sets as rs
import shade_sets as ss
import view_sets as vs
from query_sets import F, H, NO_HIT, W, bits

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUNNY = os.path.join(ROOT, "models", "big_bunny.obj")
GUARD = 0xA7


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


def lib_view(rtx, v, rect=None, rows=None):
    (w, h) = v[0]
    if rows is not None:
        rect = (0, rows[0], w, rows[1])
    return rtx.Scene.view(w, h, rect=rect, **vs.camera(v))


def where(got, want):
    return np.argwhere((got != want).any(axis=2))[:8].tolist()


def same_words(got, want, what):
    for g, w, part in zip(got, want, ("permutation", "primitive", "shading", "node", "aimed")):
        if w is None:
            continue
        bad = np.argwhere(g != w)
        assert not len(bad), "%s: %s words differ at %s" % (what, part, bad[:6].tolist())


def check_device(rtx, scene, pose, what, eye=None, tie_rank=None):
    """the rebuilt pose the device holds against the host statement: rtx_scene_rebuilt_records, and with an eye the aim
    kernels' output over it against rtx_scene_rebuilt_aimed"""
    keys, perm, t, s, n = scene.rebuilt_records(pose, tie_rank=tie_rank)
    aimed = scene.rebuilt_aimed(pose, eye) if eye is not None else None
    same_words(scene.debug_pose_rebuilt(eye=eye), (perm, t, s, n, aimed), what)


# ---------------------------------------------------------------------------------------------- 1: the words
def test_device_words_are_the_hosts_on_the_shape_scenes(rtx, orc, samples_seeded):
    torch = pytest.importorskip("torch")
    scenes = dict(rs.shape_scenes(rtx))
    rng = np.random.default_rng(22)
    spheres = np.concatenate([rng.uniform(-40, 40, (13, 3)), rng.uniform(0.5, 3.0, (13, 1))], axis=1).astype(F)
    scenes["spheres_only"] = (np.zeros((0, 9), F), spheres, np.ones(13, np.uint8), {}, np.zeros((0, 9), F))
    scenes["soup20000"] = (rtx.synthetic_mesh(20000), None, None, {}, rtx.synthetic_mesh(20000, seed=rs.SCATTER_SEED))
    eye = (0.0, 100.0, 200.0)
    for name, sc in scenes.items():
        with ps.open_small(rtx, samples_seeded, sc) as scene:
            own = np.ascontiguousarray(scene.tris.copy())
            rank = np.arange(scene.n_prims, dtype=np.uint32)[::-1].copy()
            for pose, what in ((own, "identity"), (sc[4], "posed"), (own, "identity again")):
                scene.pose_rebuilt(pose)
                check_device(rtx, scene, pose, "%s %s, host variant" % (name, what), eye=eye)
            scene.pose_rebuilt(sc[4], tie_rank=rank)
            check_device(rtx, scene, sc[4], "%s, host variant, given ranks" % name, tie_rank=rank)
            if len(own) == 0:
                continue                                            # (no vertex array to hand the device variant)
            d_pose = torch.from_numpy(np.ascontiguousarray(sc[4])).to("cuda:0")
            d_rank = torch.from_numpy(rank.view(np.int32)).to("cuda:0")
            torch.cuda.synchronize()
            stream = torch.cuda.current_stream().cuda_stream
            scene.pose_rebuilt_device(0, d_pose.data_ptr(), None, stream)
            check_device(rtx, scene, sc[4], "%s, device variant" % name, eye=eye)
            scene.pose_rebuilt_device(0, d_pose.data_ptr(), d_rank.data_ptr(), stream)
            check_device(rtx, scene, sc[4], "%s, device variant, given ranks" % name, tie_rank=rank)
            torch.cuda.synchronize()


def test_keys_saturate_outside_the_range_rule_device_variant(rtx, orc, samples_seeded):
    """rtx_scene_pose_rebuilt_device does not check the range rule: coordinates beyond M give keys in the first and the last
    cell, the permutation is still a permutation, and the words are the host statement's (which does not check it either).
    Nothing is walked here: values over such a pose are unspecified."""
    torch = pytest.importorskip("torch")
    sc = rs.shape_scenes(rtx)["soup257_ground"]
    pose = sc[4].copy()
    pose[10:40] *= F(300.0)                                # up to about 5e4: beyond M = 10,000 on either side
    pose[50:60] -= F(4.0e4)                                # (moved, not collapsed: a zero-area triangle's normal is a NaN of unspecified bits)
    pose[60:70, 0::3] = F(2.5e4)
    with ps.open_small(rtx, samples_seeded, sc) as scene:
        assert np.abs(pose).max() > scene.pose_bound()
        with pytest.raises(rtx.RtxError) as e:
            scene.pose_rebuilt(pose)                           # the host variant refuses it
        assert e.value.code == rtx.ERR_UNSUPPORTED
        d_pose = torch.from_numpy(np.ascontiguousarray(pose)).to("cuda:0")
        torch.cuda.synchronize()
        scene.pose_rebuilt_device(0, d_pose.data_ptr(), None, torch.cuda.current_stream().cuda_stream)
        check_device(rtx, scene, pose, "beyond the range rule", eye=(0.0, 100.0, 200.0))
        torch.cuda.synchronize()
        keys, perm = scene.rebuilt_records(pose)[:2]
        cells = [(keys >> np.uint64(k)) & np.uint64(0x1249249249249249) for k in (0, 1, 2)]
        assert any((c == 0).any() for c in cells) and any((c == np.uint64(0x1249249249249249)).any() for c in cells)
        assert np.array_equal(np.sort(perm), np.arange(1, scene.n_prims))


@pytest.mark.parametrize("name", ps.BUNNY_POSES)
def test_device_words_are_the_hosts_on_the_bunny(rtx, orc, samples_seeded, bunny, name):
    torch = pytest.importorskip("torch")
    pose = ps.bunny_pose(orc, name)
    st = bunny.pose_rebuilt(pose, stats=True)
    assert st["kernel_ms"] > 0 and st["rays"] == 0
    for eye in (ps.SIDE[1], vs.BUNNY_VIEWS["back"][1]):
        check_device(rtx, bunny, pose, name + ", host variant", eye=eye)
    d_pose = torch.from_numpy(pose).to("cuda:0")
    torch.cuda.synchronize()
    bunny.pose_rebuilt_device(0, d_pose.data_ptr(), None, torch.cuda.current_stream().cuda_stream)
    check_device(rtx, bunny, pose, name + ", device variant", eye=ps.SIDE[1])
    torch.cuda.synchronize()
    # the refitted pose's readers do not apply to the node-sized outputs of a rebuilt pose
    n = bunny.info()["n_nodes"]
    nodes = np.zeros((n, 8), np.uint32)
    L, u32p, f32p = rtx.rtx._lib, rtx.rtx.u32p, rtx.rtx.f32p
    assert L.rtx_debug_pose(bunny.handle, 0, None, None, nodes.ctypes.data_as(u32p)) == rtx.ERR_BAD_ARG
    eye = np.asarray(ps.SIDE[1], F)
    assert L.rtx_debug_pose_pipeline(bunny.handle, 0, eye.ctypes.data_as(f32p), None, nodes.ctypes.data_as(u32p)) == rtx.ERR_BAD_ARG
    tris = np.zeros((4969, 16), np.uint32)
    assert L.rtx_debug_pose(bunny.handle, 0, tris.ctypes.data_as(u32p), None, None) == rtx.OK
    assert np.array_equal(tris, bunny.rebuilt_records(pose)[2])
    assert np.array_equal(bunny.debug_pose_pipeline()[0], bunny.posed_pipeline_records(pose)[0])       # the planes are any pose's


# ---------------------------------------------------------------------------------------------- 2: posed frames
@pytest.mark.parametrize("name", ps.BUNNY_POSES)
def test_views_and_rows_are_the_oracle_scene_with_the_posed_vertices(rtx, orc, samples_seeded, bunny, name):
    p = ps.posed(orc, samples_seeded, name)
    view = lib_view(rtx, ps.SIDE)
    bunny.pose(p["pose"])
    refitted = bunny.render_view(view, posed=True), bunny.render_view_rows(view, posed=True)
    bunny.pose_rebuilt(p["pose"])
    rgb, shade, hits, st = bunny.render_view(view, stats=True, want_shade=True, want_hits=True, posed=True)
    assert np.array_equal(rgb, p["frame"]), "%s: bytes differ from the oracle scene at (y, x) %s" % (name, where(rgb, p["frame"]))
    assert np.array_equal(bits(shade["linear"]), bits(p["lin"])), name + ": linear differs from the oracle scene's"
    assert np.array_equal(shade["rgb8"], rgb), name
    assert np.array_equal(hits["prim"][:, :, 0], p["tri"]), name + ": hit primitives differ"
    assert st["primary_hits"] == p["stats"]["primary_hits"] and st["shadow_rays"] == p["stats"]["shadow_rays"], (name, st)
    rows, rst = bunny.render_view_rows(view, stats=True, posed=True)
    assert np.array_equal(rows, p["frame"]), "%s: rows differ from the oracle scene at (y, x) %s" % (name, where(rows, p["frame"]))
    assert rst["primary_hits"] == p["stats"]["primary_hits"] and rst["shadow_rays"] == p["stats"]["shadow_rays"] and rst["redo_tiles"] == 0
    assert np.array_equal(bunny.render_view_rows(view, posed=True), rows)                 # the aimed stream standing
    assert np.array_equal(rgb, refitted[0]) and np.array_equal(rows, refitted[1]), name + ": differs from the refitted pose's"


def test_rectangles_guarded_buffers_and_a_light(rtx, orc, samples_seeded, bunny):
    p = ps.posed(orc, samples_seeded, "turn")
    bunny.pose_rebuilt(p["pose"])
    view = lib_view(rtx, ps.SIDE)
    rgb, shade, hits = bunny.render_view(view, want_shade=True, want_hits=True, posed=True)
    s = ps.composition(orc, samples_seeded, "turn")
    assert shade.reshape(-1).tobytes() == s["shade"].tobytes(), "shade records differ from the composition on the posed oracle scene"
    qs.check_hits(hits.reshape(-1), s["hit"], ps.tables(orc, samples_seeded, "turn")["normals"], "turn: hit records")
    for rect in vs.SIDE_RECTS:                                   # rectangles off the tile grid, bytes around the output kept
        x0, y0, nx, ny = rect
        n = nx * ny * 3
        buf = np.full(64 + n + 64, GUARD, np.uint8)
        v = lib_view(rtx, ps.SIDE, rect=rect)
        rc = rtx.rtx._lib.rtx_render_view_posed(bunny.handle, 0, C.byref(v), None, buf[64:].ctypes.data, None, None, None)
        assert rc == rtx.OK, rect
        assert (buf[:64] == GUARD).all() and (buf[64 + n:] == GUARD).all(), "bytes changed around the output"
        assert np.array_equal(buf[64:64 + n].reshape(ny, nx, 3), p["frame"][y0:y0 + ny, x0:x0 + nx]), rect
    (w, h) = ps.SIDE[0]
    for y0, ny in ((3, 13), (h - 1, 1), (5, 17)):                # row windows of the pipeline
        n = ny * w * 3
        buf = np.full(64 + n + 64, GUARD, np.uint8)
        v = lib_view(rtx, ps.SIDE, rows=(y0, ny))
        rc = rtx.rtx._lib.rtx_render_view_rows_posed(bunny.handle, 0, C.byref(v), None, buf[64:].ctypes.data, None)
        assert rc == rtx.OK, (y0, ny)
        assert (buf[:64] == GUARD).all() and (buf[64 + n:] == GUARD).all(), "bytes changed around the output"
        assert np.array_equal(buf[64:64 + n].reshape(ny, w, 3), p["frame"][y0:y0 + ny]), (y0, ny)
    # under a given light: the oracle scene created with the posed vertices AND that light
    tri, count = ls.SIDE_LIGHTS[ps.POSE_LIGHT]
    light = rtx.Scene.make_light(tri, count)
    frame, ost = ps.lit_frame(orc, samples_seeded, "turn", ps.POSE_LIGHT)
    lit = bunny.render_view(view, stats=True, posed=True, light=light)
    assert np.array_equal(lit[0], frame), "lit posed view differs from the oracle scene at %s" % where(lit[0], frame)
    assert lit[1]["shadow_rays"] == ost["shadow_rays"] and (lit[0] != rgb).any()
    rows, rst = bunny.render_view_rows(view, stats=True, posed=True, light=light)
    assert np.array_equal(rows, frame), "lit posed rows differ from the oracle scene at %s" % where(rows, frame)
    assert np.array_equal(bunny.render_view_rows(view, posed=True), p["frame"])           # the scene's light afterwards


def test_the_lifted_ground_frame(rtx, orc, samples_seeded):
    L = pr.lifted(orc, samples_seeded)
    view = lib_view(rtx, pr.LIFT_VIEW)
    with pr.lift_scene(rtx, samples_seeded) as scene:
        scene.pose_rebuilt(pr.lift_pose())
        check_device(rtx, scene, pr.lift_pose(), "lifted ground", eye=pr.LIFT_VIEW[1])
        rgb, st = scene.render_view_rows(view, stats=True, posed=True)
        assert np.array_equal(rgb, L["frame"]), "bytes differ from the oracle scene at (y, x) %s" % where(rgb, L["frame"])
        assert st["primary_hits"] == L["stats"]["primary_hits"]
        assert np.array_equal(rgb, scene.render_view(view, posed=True))
        assert np.array_equal(scene.render_view_rows(view), L["still"])


def test_the_scatter_pose_and_its_counted_node_records(rtx, orc, samples_seeded, capsys):
    """The soup re-drawn with another seed: oracle bytes through the view kernel and the pipeline, over the rebuilt and the
    refitted tree; and the counted node records (RtxStats.box_tests, wave_node_visits) of the frame, rebuilt below refitted —
    the ordering the CPU's surface-area cost shows (tests/test_rebuild_host.py).  Measured, 36 x 33: view kernel 262,243
    wavefront node visits and 13.5 M box tests rebuilt against 3,490,649 and 164.0 M refitted; pipeline 161,466 and 7.4 M
    against 3,422,096 and 147.3 M."""
    fx = rs.scattered(rtx, orc, samples_seeded)
    tris, pose = rs.scatter(rtx)
    view = lib_view(rtx, rs.SCATTER_VIEW)
    assert (fx["frame"] != fx["still"]).any(axis=2).sum() >= 50
    with rs.scatter_scene(rtx, samples_seeded) as scene:
        assert np.array_equal(scene.render_view_rows(view), fx["still"])
        out = {}
        for kind, make in (("refitted", scene.pose), ("rebuilt", scene.pose_rebuilt)):
            make(pose)
            rgb, st = scene.render_view(view, stats=True, posed=True)
            rows, rst = scene.render_view_rows(view, stats=True, posed=True)
            assert np.array_equal(rgb, fx["frame"]), "%s view: differs from the oracle scene at %s" % (kind, where(rgb, fx["frame"]))
            assert np.array_equal(rows, fx["frame"]), "%s rows: differ from the oracle scene at %s" % (kind, where(rows, fx["frame"]))
            assert st["primary_hits"] == fx["frame_stats"]["primary_hits"] == rst["primary_hits"]
            out[kind] = (st, rst)
        check_device(rtx, scene, pose, "scatter", eye=rs.SCATTER_VIEW[1])
        with capsys.disabled():
            for kind, (st, rst) in out.items():
                print("\nscatter, %s: view box_tests %d wave_node_visits %d kernel_ms %.3f; rows box_tests %d wave_node_visits %d kernel_ms %.3f"
                      % (kind, st["box_tests"], st["wave_node_visits"], st["kernel_ms"], rst["box_tests"], rst["wave_node_visits"],
                         rst["kernel_ms"]))
        for k in (0, 1):
            assert out["rebuilt"][k]["wave_node_visits"] < out["refitted"][k]["wave_node_visits"], (k, out)
            assert out["rebuilt"][k]["box_tests"] < out["refitted"][k]["box_tests"], (k, out)


# ---------------------------------------------------------------------------------------------- 3: queries and shading
@pytest.mark.parametrize("name", ["turn", "tilt"])
def test_ray_queries_and_shading_on_the_rebuilt_pose(rtx, orc, samples_seeded, bunny, name):
    (ro, rd, exp), (to, tt, texp, occ) = ps.query_set(orc, samples_seeded, name)
    normals = ps.tables(orc, samples_seeded, name)["normals"]
    bunny.pose_rebuilt(ps.posed(orc, samples_seeded, name)["pose"])
    for n in (1, 63, 64, 65, 127, 129, len(ro)):
        for kw in (dict(keep_order=True), dict(force_regroup=True), dict()):
            qs.check_hits(bunny.trace_rays(ro[:n], rd[:n], posed=True, **kw), exp[:n], normals, "%s trace %d %s" % (name, n, kw))
            got = bunny.occluded_rays(to[:n], tt[:n], posed=True, **kw)
            assert np.array_equal(got, occ[:n]), (name, n, kw, np.nonzero(got != occ[:n])[0][:8])
    if name == "turn":
        s = ps.composition(orc, samples_seeded, name)
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
    bunny.pose_rebuilt(pose, reference_tree=rtx.REFTREE_ALWAYS)       # the reference's tree, its leaves through the permutation
    for kw in (dict(keep_order=True), dict(force_regroup=True)):
        qs.check_hits(bunny.trace_rays(o, d, posed=True, **kw), exp, normals, "hard rays under RTX_REFTREE_ALWAYS %s" % kw)
    (ro, rd, qexp), _ = ps.query_set(orc, samples_seeded, "turn")
    qs.check_hits(bunny.trace_rays(ro, rd, posed=True), qexp, normals, "ordinary rays under RTX_REFTREE_ALWAYS")
    # RTX_REFTREE_NEVER: the rebuilt stream with the reference's box test — some tree over these primitives; it terminates,
    # and every hit it reports is the twin's or a miss
    bunny.pose_rebuilt(pose, reference_tree=rtx.REFTREE_NEVER)
    got = bunny.trace_rays(o, d, posed=True, keep_order=True)
    hit = got["prim"] != NO_HIT
    assert np.array_equal(got["prim"][hit], twin["prim"][hit])


def test_ties_between_coincident_posed_triangles(rtx, orc, samples_seeded):
    o, d = ps.TIE_RAYS
    rgb = np.ones((3, 3), F)
    osc = orc.Scene(8, 8, ps.TIE_POSE, rgb, samples_seeded, **ps.TIE_KW)
    exp, _ = qs.oracle_hits(orc, osc, o, d, qs.HIT_DTYPE)
    with rtx.Scene(8, 8, ps.TIE_TRIS, rgb, samples_seeded[:4096], **ps.TIE_KW) as scene:
        scene.pose_rebuilt(ps.TIE_POSE, reference_tree=rtx.REFTREE_ALWAYS)
        got = scene.trace_rays(o, d, posed=True)
        assert np.array_equal(got["prim"], exp["prim"]) and np.array_equal(bits(got["t"]), bits(exp["t"]))
        scene.pose_rebuilt(ps.TIE_POSE, reference_tree=rtx.REFTREE_NEVER)
        assert scene.trace_rays(o, d, posed=True)["prim"][0] == 1              # NULL ranks: the larger index
        scene.pose_rebuilt(ps.TIE_POSE, tie_rank=np.array([5, 3, 0], np.uint32), reference_tree=rtx.REFTREE_NEVER)
        assert scene.trace_rays(o, d, posed=True)["prim"][0] == 0              # the larger tie_rank
        scene.pose_rebuilt(ps.TIE_POSE, tie_rank=np.array([2, 3, 9], np.uint32), reference_tree=rtx.REFTREE_ALWAYS)
        assert scene.trace_rays(o, d, posed=True)["prim"][0] == 1              # given ranks go before the tree's
        assert scene.trace_rays(o, d)["prim"][0] == 0
    osc.close()


@pytest.mark.parametrize("rule", ["REFTREE_NEVER", "REFTREE_ALWAYS"])
def test_hard_rays_and_the_exact_tie_through_the_pipeline(rtx, orc, samples_seeded, rule):
    """P of sequence_sets through its own axis camera: -0.0 direction components and an exact tie; the rebuilt pose's rows
    are rtx_render_view_posed's under the same rule, and under RTX_REFTREE_ALWAYS with the scene's own triangles the oracle's"""
    hs = vs.hard_scene("P", orc, samples_seeded, rtx)
    with rtx.Scene(*hs["args"], **hs["kw"]) as scene:
        v = lib_view(rtx, hs["v"])
        own = np.ascontiguousarray(scene.tris.copy())
        half = np.ascontiguousarray((own * F(0.5)).astype(F))
        frames = []
        for pose in (own, half):
            scene.pose_rebuilt(pose, reference_tree=getattr(rtx, rule))
            rgb, st = scene.render_view_rows(v, stats=True, posed=True)
            want = scene.render_view(v, posed=True)
            assert np.array_equal(rgb, want), "%s: differs from rtx_render_view_posed at %s" % (rule, where(rgb, want))
            assert st["redo_tiles"] > 0
            frames.append(rgb)
        if rule == "REFTREE_ALWAYS":
            assert np.array_equal(frames[0], hs["ref"]["frame"])
            scene.pose(own, reference_tree=rtx.REFTREE_ALWAYS)
            assert np.array_equal(scene.render_view_rows(v, posed=True), frames[0])
        assert np.array_equal(scene.render_view_rows(v), hs["ref"]["frame"])


# ---------------------------------------------------------------------------------------------- 5: spheres
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
    with rtx.Scene(*a["args"], nb_ray=2, **a["kw"]) as scene:
        view = lib_view(rtx, vs.SOUP_VIEW)
        scene.pose_rebuilt(pose, reference_tree=rtx.REFTREE_ALWAYS)
        check_device(rtx, scene, pose, "soup with spheres", eye=vs.SOUP_VIEW[1], tie_rank=scene.debug_pose_rebuilt()[2][:, 3].copy())
        got, gst = scene.render_view(view, stats=True, posed=True)
        assert np.array_equal(got, frame), where(got, frame)
        assert gst["primary_hits"] == st["primary_hits"]
        rows = scene.render_view_rows(view, posed=True)
        assert np.array_equal(rows, frame), where(rows, frame)
        assert np.array_equal(scene.render_view(view), fx["frame"])
        scene.pose_rebuilt(tris)
        assert np.array_equal(scene.render_view(view, posed=True), fx["frame"])


# ---------------------------------------------------------------------------------------------- 6: state
def test_state(rtx, orc, samples_seeded):
    view, back = lib_view(rtx, ps.SIDE), lib_view(rtx, vs.BUNNY_VIEWS["back"])
    frames = {n: ps.posed(orc, samples_seeded, n)["frame"] for n in ("identity", "turn", "shift")}
    with rtx.default_scene([BUNNY], W, H, samples_seeded) as scene, rtx.default_scene([BUNNY], W, H, samples_seeded) as other:
        usual = scene.render_rows().tobytes()
        unposed = scene.render_view_rows(view).tobytes(), scene.render_view(view).tobytes()
        # no pose, and a refitted pose: no rebuilt pose to read back
        with pytest.raises(rtx.RtxError) as e:
            scene.debug_pose_rebuilt()
        assert e.value.code == rtx.ERR_BAD_ARG
        scene.pose(ps.bunny_pose(orc, "turn"))
        with pytest.raises(rtx.RtxError) as e:
            scene.debug_pose_rebuilt()
        assert e.value.code == rtx.ERR_BAD_ARG
        # refitted -> rebuilt -> refitted on one scene, one eye standing: each pose its own frame through both paths
        for name, make in (("turn", scene.pose), ("shift", scene.pose_rebuilt), ("turn", scene.pose_rebuilt), ("shift", scene.pose),
                           ("identity", scene.pose_rebuilt), ("turn", scene.pose)):
            make(ps.bunny_pose(orc, name))
            assert np.array_equal(scene.render_view_rows(view, posed=True), frames[name]), name       # (the aimed cache was taken away)
            assert np.array_equal(scene.render_view(view, posed=True), frames[name]), name
            assert scene.render_view_rows(view).tobytes() == unposed[0], name + ": the unposed rows changed"
        same = scene.debug_pose()                                  # a refitted pose again: its readers serve, node words included
        assert all(np.array_equal(g, w) for g, w in zip(same, scene.posed_records(ps.bunny_pose(orc, "turn"))))
        # a rebuilt pose under a standing eye, another eye in between
        scene.pose_rebuilt(ps.bunny_pose(orc, "shift"))
        assert np.array_equal(scene.render_view_rows(view, posed=True), frames["shift"])
        back_unposed = scene.render_view_rows(back)
        assert np.array_equal(scene.render_view_rows(view, posed=True), frames["shift"])
        scene.pose_rebuilt(ps.bunny_pose(orc, "turn"))
        assert np.array_equal(scene.render_view_rows(view, posed=True), frames["turn"])
        assert np.array_equal(scene.render_view_rows(back), back_unposed)
        # a refused pose leaves the previous one
        with pytest.raises(rtx.RtxError) as e:
            bad = ps.bunny_pose(orc, "shift").copy()
            bad[7, 2] = 10000.5
            scene.pose_rebuilt(bad)
        assert e.value.code == rtx.ERR_UNSUPPORTED
        assert np.array_equal(scene.render_view_rows(view, posed=True), frames["turn"])
        check_device(rtx, scene, ps.bunny_pose(orc, "turn"), "after a refused pose", eye=ps.SIDE[1])
        # two live scenes, each its own pose, one rebuilt and one refitted
        other.pose(ps.bunny_pose(orc, "shift"))
        for k in range(2):
            assert np.array_equal(scene.render_view_rows(view, posed=True), frames["turn"])
            assert np.array_equal(other.render_view_rows(view, posed=True), frames["shift"])
        # the unposed bytes afterwards
        assert scene.render_rows().tobytes() == usual and other.render_rows().tobytes() == usual
        assert (scene.render_view_rows(view).tobytes(), scene.render_view(view).tobytes()) == unposed


def test_a_shrinking_and_growing_workspace(rtx, orc, samples_seeded, bunny):
    """frames of other sizes between rebuilt poses, and a scene with more nodes rebuilt than uploaded and one with fewer"""
    p = ps.posed(orc, samples_seeded, "turn")
    view, small = lib_view(rtx, ps.SIDE), lib_view(rtx, ps.TURNTABLE_VIEW)
    turns = ps.turntable(orc, samples_seeded)
    assert bunny.rebuilt_counts() != bunny.info()["n_nodes"]
    bunny.pose_rebuilt(p["pose"])
    assert np.array_equal(bunny.render_view_rows(view, posed=True), p["frame"])
    bunny.pose_rebuilt(turns[0][0])
    assert np.array_equal(bunny.render_view_rows(small, posed=True), turns[0][1])
    bunny.pose(p["pose"])
    assert np.array_equal(bunny.render_view_rows(view, posed=True), p["frame"])
    bunny.pose_rebuilt(turns[1][0])
    assert np.array_equal(bunny.render_view_rows(small, posed=True), turns[1][1])
    assert np.array_equal(bunny.render_view(small, posed=True), turns[1][1])
    with ps.open_small(rtx, samples_seeded, ps.small_scenes(rtx)["soup257_ground"], leaf_max=1) as more, \
            ps.open_small(rtx, samples_seeded, ps.small_scenes(rtx)["soup257_ground"], leaf_max=16) as fewer:
        pose = ps.small_scenes(rtx)["soup257_ground"][4]
        for scene in (more, fewer):
            for make in (scene.pose_rebuilt, scene.pose, scene.pose_rebuilt):
                make(pose)
            check_device(rtx, scene, pose, "leaf_max", eye=(0.0, 100.0, 200.0))


# ---------------------------------------------------------------------------------------------- 7: device-resident
def test_device_resident_rebuilt_pose_and_posed_launches_on_one_stream(rtx, orc, samples_seeded, bunny):
    torch = pytest.importorskip("torch")
    assert torch.cuda.is_available(), "torch sees no GPU"
    turn, shift = (ps.posed(orc, samples_seeded, n) for n in ("turn", "shift"))
    view = lib_view(rtx, ps.SIDE)
    n = view.ny * view.width * 3
    stream = torch.cuda.Stream(device="cuda:0")
    assert stream.cuda_stream != torch.cuda.default_stream().cuda_stream
    with torch.cuda.stream(stream):
        d_turn, d_shift = (torch.from_numpy(p["pose"].copy()).to("cuda:0") for p in (turn, shift))
        bufs = [torch.full((n + 16,), 0xAA, dtype=torch.uint8, device="cuda:0") for _ in range(4)]
        counters = torch.zeros(8, dtype=torch.int64, device="cuda:0")
        stream.synchronize()
        # a rebuilt pose, its rows, a refitted pose, its view, a rebuilt pose, its rows twice: one stream, nothing waited for
        bunny.pose_rebuilt_device(0, d_turn.data_ptr(), None, stream.cuda_stream)
        bunny.render_view_rows_device(0, view, bufs[0].data_ptr(), bufs[0].numel(), stream.cuda_stream, counters.data_ptr(), posed=True)
        bunny.pose_device(0, d_shift.data_ptr(), None, stream.cuda_stream)
        bunny.render_view_device(0, view, bufs[1].data_ptr(), None, None, stream.cuda_stream, posed=True)
        bunny.pose_rebuilt_device(0, d_shift.data_ptr(), None, stream.cuda_stream)
        bunny.render_view_rows_device(0, view, bufs[2].data_ptr(), bufs[2].numel(), stream.cuda_stream, counters.data_ptr(), posed=True)
        bunny.render_view_rows_device(0, view, bufs[3].data_ptr(), bufs[3].numel(), stream.cuda_stream, posed=True)
        # ... and a host posed call right behind them, on the library's stream: it waits for the event
        host = bunny.render_view_rows(view, posed=True)
        assert np.array_equal(host, shift["frame"])
        stream.synchronize()
        for p, b in zip((turn, shift, shift, shift), bufs):
            out = b.cpu().numpy()
            assert out[:n].tobytes() == p["frame"].tobytes() and (out[n:] == 0xAA).all()
        got = counters.cpu().numpy()
        assert int(got[0]) == turn["stats"]["primary_hits"] + shift["stats"]["primary_hits"], got
        # the ray-batch device forms against the posed oracle scene (the device holds `shift`, rebuilt)
        (ro, rd, exp), (to, tt, _, occ) = ps.query_set(orc, samples_seeded, "shift")
        m = len(ro)
        d_o, d_d, d_to, d_tt = (torch.from_numpy(np.ascontiguousarray(x)).to("cuda:0") for x in (ro, rd, to, tt))
        d_hits = torch.zeros(m * 32, dtype=torch.uint8, device="cuda:0")
        d_occ = torch.zeros(m, dtype=torch.uint8, device="cuda:0")
        stream.synchronize()
        bunny.trace_rays_device(0, m, d_o.data_ptr(), d_d.data_ptr(), d_hits.data_ptr(), stream.cuda_stream, force_regroup=True, posed=True)
        bunny.occluded_rays_device(0, m, d_to.data_ptr(), d_tt.data_ptr(), d_occ.data_ptr(), stream.cuda_stream, posed=True)
        # a host rebuilt pose right behind them: it waits for the launches that still read the pose it replaces
        bunny.pose_rebuilt(turn["pose"])
        stream.synchronize()
        qs.check_hits(d_hits.cpu().numpy().view(rtx.rtx.RAY_HIT_DTYPE), exp, None, "rtx_trace_rays_posed_device")
        assert np.array_equal(d_occ.cpu().numpy(), occ)
    assert np.array_equal(bunny.render_view_rows(view, posed=True), turn["frame"])
    assert np.array_equal(bunny.render_view_rows(view), ps.posed(orc, samples_seeded, "identity")["frame"])


def test_four_turns_of_the_mesh(rtx, orc, samples_seeded, bunny):
    view = lib_view(rtx, ps.TURNTABLE_VIEW)
    for deg, (pose, frame) in zip(ps.TURNTABLE_DEGREES, ps.turntable(orc, samples_seeded)):
        bunny.pose_rebuilt(pose)
        got = bunny.render_view_rows(view, posed=True)
        assert np.array_equal(got, frame), "turn %g: differs at %s" % (deg, where(got, frame))
        assert np.array_equal(bunny.render_view(view, posed=True), frame), deg
