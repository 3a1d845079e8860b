"""GPU parity of a pose by affine moves made on the device (rtx_scene_pose_moved, rtx_scene_pose_moved_device: the move
kernel and the overlay and pose or rebuild kernels behind it): the arrays the move kernel writes word for word against
the host statement rtx_scene_moved_prims, the pose's words against rtx_scene_pose_prims_records of those arrays, and
every posed call over such a pose against an ORACLE SCENE CREATED WITH THE STATED PRIMITIVES and against
rtx_scene_pose_prims with those arrays (tests/moves_sets.py, whose conditions tests/test_moves_sets.py asserts without a
GPU).  Every comparison is for equal bits or bytes."""
import importlib

import numpy as np
import pytest

import moves_sets as mv
import prims_sets as pm
import query_sets as qs
import shade_sets as ss
import view_sets as vs
from query_sets import F, NO_HIT, bits

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def rtx():
    mod = importlib.import_module("ray-tracer-rust_amd")
    assert mod.device_count() >= 1, "no HIP device: the product path has no CPU fallback"
    return mod


@pytest.fixture(scope="module")
def yard(rtx, samples_seeded):
    with pm.open_yard(rtx, samples_seeded) as s:
        yield s


def lib_view(rtx, rect=None, v=pm.YARD_VIEW):
    (w, h) = v[0]
    return rtx.Scene.view(w, h, rect=rect, **vs.camera(v))


def where(got, want):
    return np.argwhere((got != want).any(axis=2))[:8].tolist()


def same_arrays(got, want, what):
    for g, w, part in zip(got, want, ("vertex", "sphere")):
        bad = np.argwhere(bits(g) != bits(w))
        assert not len(bad), "%s: %s words differ from the host statement's at %s" % (what, part, bad[:6].tolist())


def same_words(got, want, what):
    for g, w, part in zip(got, want, ("primitive", "shading", "node")):
        bad = np.argwhere(g != w)
        assert not len(bad), "%s: %s words differ at %s" % (what, part, bad[:6].tolist())


def check_pose(scene, given, what, rebuilt, tie_rank=None):
    """the pose the device holds against rtx_scene_pose_prims_records of the statement's arrays"""
    if rebuilt:
        _, perm, t, s, n = scene.pose_prims_records(rebuilt=True, tie_rank=tie_rank, **given)
        dperm, dt, ds, dn, _ = scene.debug_pose_rebuilt()
        assert np.array_equal(dperm, perm), what + ": permutation"
        same_words((dt, ds, dn), (t, s, n), what + ", rebuilt")
    else:
        same_words(scene.debug_pose(), scene.pose_prims_records(tie_rank=tie_rank, **given), what + ", refitted")


def on_device(torch, kw, guard=0):
    """the pose's arrays on the device -> (keywords of rtx.Scene.pose_moved_device, the tensors that keep them alive);
    guard: so many trailing NaN entries behind moves and radius_scale"""
    keep = {}
    for k in ("moves", "group", "radius_scale", "rgb", "sphere_rgb"):
        a = kw.get(k)
        if a is None:
            continue
        a = np.ascontiguousarray(a)
        if guard and k in ("moves", "radius_scale"):
            a = np.concatenate([a, np.full((guard,) + a.shape[1:], np.nan, F)])
        keep[k] = torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).to("cuda:0")
    torch.cuda.synchronize()
    names = dict(moves="d_moves_ptr", group="d_group_ptr", radius_scale="d_radius_scale_ptr", rgb="d_rgb_ptr", sphere_rgb="d_sphere_rgb_ptr")
    out = {names[k]: t.data_ptr() for k, t in keep.items()}
    out["n_moves"] = len(kw["moves"])
    return out, keep


# ---------------------------------------------------------------------------------------------- 1: the device's arrays
@pytest.mark.parametrize("name", mv.POSES)
def test_the_devices_arrays_and_the_pose_are_the_host_statements_on_the_yard(rtx, samples_seeded, yard, name):
    torch = pytest.importorskip("torch")
    kw = mv.moves(rtx, name)
    want = yard.moved_prims(**mv.statement_kw(kw))
    stated = mv.stated(rtx, samples_seeded, name)
    assert np.array_equal(bits(want[0]), bits(stated["tris"])) and np.array_equal(bits(want[1]), bits(stated["spheres"]))
    given = mv.given(rtx, samples_seeded, name)
    rank = np.arange(pm.N_PRIMS, dtype=np.uint32)[::-1].copy()
    d_rank = torch.from_numpy(rank.view(np.int32)).to("cuda:0")
    dkw, keep = on_device(torch, kw)
    stream = torch.cuda.current_stream().cuda_stream
    for rebuilt in (False, True):
        st = yard.pose_moved(rebuilt=rebuilt, stats=True, **kw)
        assert st["kernel_ms"] > 0 and st["rays"] == 0
        same_arrays(yard.debug_moved_prims(), want, name + ", host variant")
        check_pose(yard, given, name + ", host variant", rebuilt)
        yard.pose_moved(rebuilt=rebuilt, tie_rank=rank, **kw)
        check_pose(yard, given, name + ", host variant, given ranks", rebuilt, tie_rank=rank)
        yard.pose(pm.yard(rtx)["tris"])                                 # (a host pose between: the buffers are reused)
        yard.pose_moved_device(0, rebuilt=rebuilt, stream=stream, **dkw)
        same_arrays(yard.debug_moved_prims(), want, name + ", device variant")
        check_pose(yard, given, name + ", device variant", rebuilt)
        yard.pose_moved_device(0, rebuilt=rebuilt, stream=stream, d_tie_rank_ptr=d_rank.data_ptr(), **dkw)
        check_pose(yard, given, name + ", device variant, given ranks", rebuilt, tie_rank=rank)
    torch.cuda.synchronize()


def test_the_devices_arrays_on_the_count_scenes(rtx, samples_seeded):
    """255, 256 and 257 primitives, every third a sphere (a workgroup of the move kernel ends inside the vertices, at
    their end and among the spheres), and `many`: a move per primitive"""
    torch = pytest.importorskip("torch")
    stream = torch.cuda.current_stream().cuda_stream
    for name, sc, kw in mv.count_cases(rtx):
        with pm.open_sized(rtx, samples_seeded, sc) as scene:
            with pytest.raises(rtx.RtxError) as e:                      # the move kernel never ran on this scene
                scene.debug_moved_prims()
            assert e.value.code == rtx.ERR_BAD_ARG
            want = scene.moved_prims(**kw)
            given = dict(v0v1v2=want[0], spheres=want[1], rgb=None, sphere_rgb=None)
            dkw, keep = on_device(torch, kw)
            for rebuilt in (False, True):
                scene.pose_moved(rebuilt=rebuilt, **kw)
                same_arrays(scene.debug_moved_prims(), want, "%s, host variant" % name)
                check_pose(scene, given, "%s, host variant" % name, rebuilt)
                scene.pose_moved_device(0, rebuilt=rebuilt, stream=stream, **dkw)
                same_arrays(scene.debug_moved_prims(), want, "%s, device variant" % name)
                check_pose(scene, given, "%s, device variant" % name, rebuilt)
            # NULL group and NULL radius_scale: every primitive follows move 0 — too far for these scenes' bound as a host
            # call's input would be checked, so a gentle one
            gentle = dict(moves=mv.translation((0.5, -0.25, 0.125)).reshape(1, 12), group=None, radius_scale=None)
            want = scene.moved_prims(**gentle)
            scene.pose_moved(**gentle)
            same_arrays(scene.debug_moved_prims(), want, "%s, NULL group, host variant" % name)
            dkw, keep = on_device(torch, gentle)
            scene.pose_moved_device(0, stream=stream, **dkw)
            same_arrays(scene.debug_moved_prims(), want, "%s, NULL group, device variant" % name)
            torch.cuda.synchronize()


def test_out_of_range_groups_leave_the_primitive_as_created(rtx, samples_seeded, yard):
    """the device variant reads whatever the group array holds: n_moves, n_moves + 1 and 0xFFFFFFFE are taken as
    RTX_MOVE_NONE.  Eight NaN entries stand behind the device's moves and radius_scale, so an index that was not compared
    against n_moves shows as NaN words, never as a read out of bounds; the read-back writes its two arrays and no byte
    behind them"""
    torch = pytest.importorskip("torch")
    stream = torch.cuda.current_stream().cuda_stream
    for name in ("all", "balls", "shear"):
        kw = mv.moves(rtx, name)
        n_moves = len(kw["moves"])
        g = kw["group"].copy()
        wild = np.zeros(pm.N_PRIMS, bool)
        wild[[0, 1, 2, 9, 20, 21, 33, 45]] = True                      # triangles and spheres (Vec positions 2, 9, 21, 45)
        g[wild] = np.array([n_moves, n_moves + 1, 0xFFFFFFFE], np.uint32)[np.arange(wild.sum()) % 3]
        as_none = g.copy()
        as_none[wild] = mv.NONE
        want = yard.moved_prims(kw["moves"], as_none, kw["radius_scale"])
        created = pm.yard(rtx)
        tri_of = np.cumsum(pm.kinds() == 0) - 1
        sphere_of = np.cumsum(pm.kinds() != 0) - 1
        for at in np.nonzero(wild)[0]:
            if pm.kinds()[at]:
                assert np.array_equal(bits(want[1][sphere_of[at]]), bits(created["spheres"][sphere_of[at]]))
            else:
                assert np.array_equal(bits(want[0][tri_of[at]]), bits(created["tris"][tri_of[at]]))
        dkw, keep = on_device(torch, dict(kw, group=g), guard=8)
        for rebuilt in (False, True):
            yard.pose_moved_device(0, rebuilt=rebuilt, stream=stream, **dkw)
            v = np.full(41 * 9 + 16, 7.5, F)
            s = np.full(5 * 4 + 16, 7.5, F)
            f32p = rtx.rtx.f32p
            assert rtx.rtx._lib.rtx_debug_moved_prims(yard.handle, 0, v.ctypes.data_as(f32p), s.ctypes.data_as(f32p)) == rtx.OK
            assert (v[41 * 9:] == 7.5).all() and (s[5 * 4:] == 7.5).all()
            got = v[:41 * 9].reshape(41, 9), s[:20].reshape(5, 4)
            assert np.isfinite(got[0]).all() and np.isfinite(got[1]).all(), name + ": a guard entry was read"
            same_arrays(got, want, name + ", wild groups")
            check_pose(yard, dict(v0v1v2=want[0], spheres=want[1], rgb=kw["rgb"], sphere_rgb=kw["sphere_rgb"]), name + ", wild groups",
                       rebuilt)
        torch.cuda.synchronize()
        for k, t in keep.items():                                       # the caller's arrays are read only
            if k in ("moves", "radius_scale"):
                assert torch.isnan(t[-8:]).all(), k


# ---------------------------------------------------------------------------------------------- 2: every posed call
def posed_calls(rtx, scene, light):
    """every posed call on the scene's standing pose -> dict of results"""
    view = lib_view(rtx)
    out = {}
    out["rgb"], out["shade"], out["hits"], out["view_stats"] = scene.render_view(view, stats=True, want_shade=True, want_hits=True, posed=True)
    rect = (3, 5, 13, 7)                                                # off the 8 x 8 tile grid
    out["rect"] = scene.render_view(lib_view(rtx, rect=rect), want_shade=True, want_hits=True, posed=True)
    out["rows"], out["rows_stats"] = scene.render_view_rows(view, stats=True, posed=True)
    out["window"] = scene.render_view_rows(lib_view(rtx, rect=(0, 3, 24, 9)), posed=True)
    out["lit"] = scene.render_view_rows(view, posed=True, light=light)
    out["lit_view"] = scene.render_view(view, posed=True, light=light)
    return out


def same_calls(a, b, what):
    for k in a:
        x, y = a[k], b[k]
        if isinstance(x, dict):
            assert {n: x[n] for n in ("primary_hits", "shadow_rays", "rays")} == {n: y[n] for n in ("primary_hits", "shadow_rays", "rays")}, (what, k)
        elif isinstance(x, tuple):
            assert all(p.tobytes() == q.tobytes() for p, q in zip(x, y)), (what, k)
        else:
            assert x.tobytes() == y.tobytes(), "%s: %s differs from rtx_scene_pose_prims' over the stated arrays" % (what, k)


@pytest.mark.parametrize("name", mv.CHANGING)
def test_views_and_rows_are_the_oracle_scene_and_the_prims_pose(rtx, orc, samples_seeded, yard, name):
    p = mv.posed(orc, rtx, samples_seeded, name)
    kw = mv.moves(rtx, name)
    given = mv.given(rtx, samples_seeded, name)
    tri, count = pm.POSE_LIGHT
    light = rtx.Scene.make_light(tri, count)
    lit, lit_stats = mv.lit_frame(orc, rtx, samples_seeded, name)
    assert (lit != p["frame"]).any()
    results = []
    for rebuilt in (False, True):
        what = "%s, %s" % (name, "rebuilt" if rebuilt else "refitted")
        yard.pose_moved(rebuilt=rebuilt, **kw)
        got = posed_calls(rtx, yard, light)
        assert np.array_equal(got["rgb"], p["frame"]), "%s: bytes differ from the oracle scene at (y, x) %s" % (what, where(got["rgb"], p["frame"]))
        assert np.array_equal(bits(got["shade"]["linear"]), bits(p["lin"])), what + ": linear differs from the oracle scene's"
        assert np.array_equal(got["shade"]["rgb8"], got["rgb"]), what
        assert np.array_equal(got["hits"]["prim"][:, :, 0], p["tri"]), what + ": hit primitives differ"
        for st in (got["view_stats"], got["rows_stats"]):
            assert st["primary_hits"] == p["stats"]["primary_hits"] and st["shadow_rays"] == p["stats"]["shadow_rays"], (what, st)
        x0, y0, nx, ny = 3, 5, 13, 7
        assert np.array_equal(got["rect"][0], p["frame"][y0:y0 + ny, x0:x0 + nx]), what + ": rectangle"
        assert got["rect"][1].tobytes() == np.ascontiguousarray(got["shade"][y0:y0 + ny, x0:x0 + nx]).tobytes(), what
        assert got["rect"][2].tobytes() == np.ascontiguousarray(got["hits"][y0:y0 + ny, x0:x0 + nx]).tobytes(), what
        assert np.array_equal(got["rows"], p["frame"]), "%s: rows differ from the oracle scene at (y, x) %s" % (what, where(got["rows"], p["frame"]))
        assert np.array_equal(got["window"], p["frame"][3:12]), what + ": row window"
        assert np.array_equal(got["lit"], lit) and np.array_equal(got["lit_view"], lit), what + ": under a given light"
        assert np.array_equal(yard.render_view_rows(lib_view(rtx), posed=True), p["frame"])          # the scene's light afterwards
        yard.pose_prims(rebuilt=rebuilt, **given)
        same_calls(got, posed_calls(rtx, yard, light), what)
        results.append(got)
    same_calls(results[0], results[1], name + ": refitted against rebuilt")


def test_guarded_buffers_behind_a_rectangle_and_a_row_window(rtx, orc, samples_seeded, yard):
    torch = pytest.importorskip("torch")
    p = mv.posed(orc, rtx, samples_seeded, "all")
    stream = torch.cuda.current_stream().cuda_stream
    yard.pose_moved(**mv.moves(rtx, "all"))
    x0, y0, nx, ny = 3, 5, 13, 7
    n = nx * ny * 3
    buf = torch.full((n + 16,), 0xAA, dtype=torch.uint8, device="cuda:0")
    yard.render_view_device(0, lib_view(rtx, rect=(x0, y0, nx, ny)), buf.data_ptr(), None, None, stream, posed=True)
    rows = torch.full((9 * 24 * 3 + 16,), 0xAA, dtype=torch.uint8, device="cuda:0")
    yard.render_view_rows_device(0, lib_view(rtx, rect=(0, 3, 24, 9)), rows.data_ptr(), rows.numel(), stream, posed=True)
    torch.cuda.synchronize()
    out = buf.cpu().numpy()
    assert out[:n].tobytes() == np.ascontiguousarray(p["frame"][y0:y0 + ny, x0:x0 + nx]).tobytes() and (out[n:] == 0xAA).all()
    out = rows.cpu().numpy()
    assert out[:9 * 24 * 3].tobytes() == np.ascontiguousarray(p["frame"][3:12]).tobytes() and (out[9 * 24 * 3:] == 0xAA).all()


@pytest.mark.parametrize("name", mv.CHANGING)
def test_ray_queries_and_shading_over_a_moved_pose(rtx, orc, samples_seeded, yard, name):
    (ro, rd, exp), (to, tt, texp, occ) = mv.query_set(orc, rtx, samples_seeded, name)
    tb = mv.tables(orc, rtx, samples_seeded, name)
    s = mv.composition(orc, rtx, samples_seeded, name)
    kw = mv.moves(rtx, name)
    given = mv.given(rtx, samples_seeded, name)
    for rebuilt in (False, True):
        got = []
        for moved in (True, False):
            if moved:
                yard.pose_moved(rebuilt=rebuilt, **kw)
            else:
                yard.pose_prims(rebuilt=rebuilt, **given)
            raw = []
            for n in (63, 64, 65, len(ro)):
                for order in (dict(keep_order=True), dict(force_regroup=True)):
                    hits = yard.trace_rays(ro[:n], rd[:n], posed=True, **order)
                    qs.check_hits(hits, exp[:n], None, "%s trace %d %s" % (name, n, order))
                    qs.check_normals(hits, exp[:n], tb["normals"], pm.kinds(), "%s trace %d %s" % (name, n, order))
                    o = yard.occluded_rays(to[:n], tt[:n], posed=True, **order)
                    assert np.array_equal(o, occ[:n]), (name, n, order, np.nonzero(o != occ[:n])[0][:8])
                    raw += [hits.tobytes(), o.tobytes()]
            for n0, n in ((0, 63), (100, 64), (250, 65)):            # pixels of the yard view: render_pixel for a batch
                part = ss.take(s, np.arange(n0, n0 + n))
                for order in (dict(keep_order=True), dict(force_regroup=True)):
                    shade, hits = yard.shade_rays(part["origins"], part["directions"], want_hits=True, posed=True, **order)
                    assert shade.tobytes() == part["shade"].tobytes(), (name, n0, n, order)
                    raw += [shade.tobytes(), hits.tobytes()]
            got.append(raw)
        assert got[0] == got[1], "%s: a moved pose and rtx_scene_pose_prims of the stated arrays differ" % name


# ---------------------------------------------------------------------------------------------- 3: the tree rules
def test_hard_rays_onto_the_turned_cluster_follow_the_reference_tree_rule(rtx, orc, samples_seeded, yard):
    o, d, exp, twin = mv.hard_rays(orc, rtx, samples_seeded)
    kw = mv.moves(rtx, "turn")
    (ro, rd, qexp), _ = mv.query_set(orc, rtx, samples_seeded, "turn")
    for rebuilt in (False, True):
        yard.pose_moved(rebuilt=rebuilt, reference_tree=rtx.REFTREE_ALWAYS, **kw)    # the oracle's own tree over the STATED boxes
        for order in (dict(keep_order=True), dict(force_regroup=True)):
            qs.check_hits(yard.trace_rays(o, d, posed=True, **order), exp, None, "hard rays under RTX_REFTREE_ALWAYS %s" % order)
        qs.check_hits(yard.trace_rays(ro, rd, posed=True), qexp, None, "ordinary rays under RTX_REFTREE_ALWAYS")
        yard.pose_moved(rebuilt=rebuilt, reference_tree=rtx.REFTREE_NEVER, **kw)
        # RTX_REFTREE_NEVER: the pose's stream with the reference's box test — some tree over these primitives; it
        # terminates, and what it reports is a hit of the ray, so never nearer than the twin's closest one
        got = yard.trace_rays(o, d, posed=True, keep_order=True)
        hit = got["prim"] != NO_HIT
        assert (twin["prim"][hit] != NO_HIT).all() and (got["t"][hit] >= twin["t"][hit]).all()
        assert np.array_equal(got["prim"][hit & (got["t"] == twin["t"])], twin["prim"][hit & (got["t"] == twin["t"])])


def test_an_exact_tie_between_a_sphere_a_move_brings_and_a_triangle(rtx, orc, samples_seeded):
    o, d = pm.TIE_RAY
    rgb = np.ones((2, 3), F)
    osc = orc.Scene(8, 8, pm.TIE_TRIS, rgb, samples_seeded[:4096], spheres=pm.TIE_MOVED, kinds=pm.TIE_KINDS, **pm.TIE_KW)
    exp, _ = qs.oracle_hits(orc, osc, o, d, qs.HIT_DTYPE)
    osc.close()
    kw = mv.TIE_MOVES
    with rtx.Scene(8, 8, pm.TIE_TRIS, rgb, samples_seeded[:4096], spheres=pm.TIE_SPHERES, kinds=pm.TIE_KINDS, **pm.TIE_KW) as scene:
        v, s = scene.moved_prims(**kw)
        assert np.array_equal(bits(s), bits(pm.TIE_MOVED)) and np.array_equal(bits(v), bits(pm.TIE_TRIS))
        for rebuilt in (False, True):
            scene.pose_moved(rebuilt=rebuilt, reference_tree=rtx.REFTREE_ALWAYS, **kw)
            got = scene.trace_rays(o, d, posed=True)
            assert np.array_equal(got["prim"], exp["prim"]) and np.array_equal(bits(got["t"]), bits(exp["t"])), rebuilt
            scene.pose_moved(rebuilt=rebuilt, reference_tree=rtx.REFTREE_NEVER, **kw)
            assert scene.trace_rays(o, d, posed=True)["prim"][0] == 1          # NULL ranks: the larger index, the sphere
            scene.pose_moved(rebuilt=rebuilt, tie_rank=np.array([5, 3, 0], np.uint32), **kw)
            assert scene.trace_rays(o, d, posed=True)["prim"][0] == 0          # the larger tie_rank, the triangle
            scene.pose_moved(rebuilt=rebuilt, tie_rank=np.array([2, 3, 9], np.uint32), reference_tree=rtx.REFTREE_ALWAYS, **kw)
            assert scene.trace_rays(o, d, posed=True)["prim"][0] == 1          # given ranks go before the tree's
            assert scene.trace_rays(o, d)["prim"][0] == 0                      # unposed: the sphere is elsewhere


# ---------------------------------------------------------------------------------------------- 4: state
def test_sequences(rtx, orc, samples_seeded):
    view = lib_view(rtx)
    frames = {n: mv.posed(orc, rtx, samples_seeded, n)["frame"] for n in mv.POSES}
    y = pm.yard(rtx)
    with pm.open_yard(rtx, samples_seeded) as scene, pm.open_yard(rtx, samples_seeded) as other:
        usual = scene.render_rows().tobytes()
        unposed = scene.render_view_rows(view).tobytes(), scene.render_view(view).tobytes()
        # moved -> plain rtx_scene_pose -> moved, under a standing eye
        turned = mv.stated(rtx, samples_seeded, "turn")["tris"]
        scene.pose_moved(**mv.moves(rtx, "all"))
        assert np.array_equal(scene.render_view_rows(view, posed=True), frames["all"])
        scene.pose(turned)                                          # spheres and colours are the uploaded ones again
        assert np.array_equal(scene.render_view_rows(view, posed=True), frames["turn"])
        with pytest.raises(rtx.RtxError) as e:                      # ... and the move kernel's arrays are gone
            scene.debug_moved_prims()
        assert e.value.code == rtx.ERR_BAD_ARG
        scene.pose_moved(rebuilt=True, **mv.moves(rtx, "balls"))
        assert np.array_equal(scene.render_view_rows(view, posed=True), frames["balls"])
        assert np.array_equal(scene.render_view(view, posed=True), frames["balls"])
        # a refused moved pose leaves the previous pose standing
        bad = mv.moves(rtx, "turn")
        with pytest.raises(rtx.RtxError) as e:
            scene.pose_moved(**dict(bad, group=None))               # the ground turns: its corner leaves the bound
        assert e.value.code == rtx.ERR_UNSUPPORTED
        g = bad["group"].copy()
        g[7] = 1
        with pytest.raises(rtx.RtxError) as e:
            scene.pose_moved(**dict(bad, group=g))
        assert e.value.code == rtx.ERR_BAD_ARG
        assert np.array_equal(scene.render_view_rows(view, posed=True), frames["balls"])
        balls = mv.stated(rtx, samples_seeded, "balls")
        same_arrays(scene.debug_moved_prims(), (balls["tris"], balls["spheres"]), "after a refused pose")
        # `same` equals the unposed calls; `unit` too on this yard (no -0.0 coordinate)
        for name in ("same", "unit"):
            scene.pose_moved(**mv.moves(rtx, name))
            assert (scene.render_view_rows(view, posed=True).tobytes(), scene.render_view(view, posed=True).tobytes()) == unposed, name
        scene.pose(y["tris"])
        plain = scene.debug_pose()
        scene.pose_moved(**mv.moves(rtx, "same"))
        same_words(scene.debug_pose(), plain, "`same` against rtx_scene_pose of the created vertices")
        # two live scenes, each its own pose
        scene.pose_moved(**mv.moves(rtx, "shear"))
        other.pose_moved(rebuilt=True, **mv.moves(rtx, "turn"))
        for k in range(2):
            assert np.array_equal(scene.render_view_rows(view, posed=True), frames["shear"])
            assert np.array_equal(other.render_view_rows(view, posed=True), frames["turn"])
        # the unposed calls give the scene's usual bytes
        assert scene.render_rows().tobytes() == usual and other.render_rows().tobytes() == usual
        assert (scene.render_view_rows(view).tobytes(), scene.render_view(view).tobytes()) == unposed


def test_many_moves_on_their_scene(rtx, orc, samples_seeded):
    """257 moves, one per primitive: the frame against the oracle scene created with the stated primitives"""
    name, sc, kw = mv.count_cases(rtx)[-1]
    assert name == "many"
    cam = dict(eye=(0.0, 100.0, 200.0), look_at=(-15.0, 100.0, 0.0), up=vs.UP, distance=30.0)
    view = rtx.Scene.view(24, 16, **cam)
    with pm.open_sized(rtx, samples_seeded, sc) as scene:
        v, s = scene.moved_prims(**kw)
        osc = orc.Scene(24, 16, v, sc["rgb"], samples_seeded[:4096], spheres=s, sphere_rgb=sc["sphere_rgb"], kinds=sc["kinds"],
                        nb_ray=1, nb_light_sample=4, **cam)
        want, _ = osc.render_rows(mode=orc.MODE_BVH)
        osc.close()
        usual = scene.render_rows().tobytes()
        still = scene.render_view(view)
        for rebuilt in (False, True):
            scene.pose_moved(rebuilt=rebuilt, **kw)
            assert np.array_equal(scene.render_view(view, posed=True), want), where(scene.render_view(view, posed=True), want)
            assert np.array_equal(scene.render_view_rows(view, posed=True), want)
        assert (want != still).any() and (want != want[0, 0]).any()
        assert scene.render_rows().tobytes() == usual and np.array_equal(scene.render_view(view), still)


# ---------------------------------------------------------------------------------------------- 5: device-resident, turns
def test_device_resident_moved_poses_and_posed_rows_on_one_stream(rtx, orc, samples_seeded, yard):
    torch = pytest.importorskip("torch")
    assert torch.cuda.is_available(), "torch sees no GPU"
    view = lib_view(rtx)
    n = view.ny * view.width * 3
    names = ("turn", "all")
    frames = [mv.posed(orc, rtx, samples_seeded, k)["frame"] for k in names]
    stream = torch.cuda.Stream(device="cuda:0")
    assert stream.cuda_stream != torch.cuda.default_stream().cuda_stream
    with torch.cuda.stream(stream):
        on = [on_device(torch, mv.moves(rtx, k)) for k in names]
        bufs = [torch.full((n + 16,), 0xAA, dtype=torch.uint8, device="cuda:0") for _ in range(3)]
        stream.synchronize()
        # a refitted moved pose, its rows, a rebuilt one, its rows twice: one stream, nothing waited for
        yard.pose_moved_device(0, stream=stream.cuda_stream, **on[0][0])
        yard.render_view_rows_device(0, view, bufs[0].data_ptr(), bufs[0].numel(), stream.cuda_stream, posed=True)
        yard.pose_moved_device(0, rebuilt=True, stream=stream.cuda_stream, **on[1][0])
        yard.render_view_rows_device(0, view, bufs[1].data_ptr(), bufs[1].numel(), stream.cuda_stream, posed=True)
        yard.render_view_rows_device(0, view, bufs[2].data_ptr(), bufs[2].numel(), stream.cuda_stream, posed=True)
        # ... and a host posed call right behind them, on the library's stream: it waits for the event
        assert np.array_equal(yard.render_view_rows(view, posed=True), frames[1])
        # ... and a host moved pose: it waits for the launches that still read the pose and the arrays it replaces
        yard.pose_moved(**mv.moves(rtx, "balls"))
        stream.synchronize()
        for f, b in zip((frames[0], frames[1], frames[1]), bufs):
            out = b.cpu().numpy()
            assert out[:n].tobytes() == f.tobytes() and (out[n:] == 0xAA).all()
    assert np.array_equal(yard.render_view_rows(view, posed=True), mv.posed(orc, rtx, samples_seeded, "balls")["frame"])


def test_four_turns_of_the_cluster(rtx, orc, samples_seeded, yard):
    """a turntable: four turns, 48 bytes each; every frame against the oracle scene created with the stated vertices"""
    view = lib_view(rtx)
    group = mv.moves(rtx, "turn")["group"]
    seen = []
    for k, degrees in enumerate((90.0, 180.0, 270.0, 360.0)):
        kw = dict(moves=mv.turn_move(rtx, degrees).reshape(1, 12), group=group)
        v, s = yard.moved_prims(**kw)
        prims = dict(pm.yard_pose(rtx, "identity"), tris=v, spheres=s)
        r = pm.render(orc, samples_seeded, prims)
        r["osc"].close()
        yard.pose_moved(rebuilt=bool(k % 2), **kw)
        got = yard.render_view_rows(view, posed=True)
        assert np.array_equal(got, r["frame"]), "turn %d differs from the oracle scene at %s" % (k, where(got, r["frame"]))
        assert np.array_equal(yard.render_view(view, posed=True), r["frame"])
        seen.append(got.tobytes())
    assert len(set(seen)) >= 3
