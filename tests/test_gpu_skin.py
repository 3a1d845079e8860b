"""GPU parity of a skinned pose (rtx_scene_skin, rtx_scene_pose_skinned, rtx_scene_pose_skinned_device: the skin kernel and
the overlay and pose or rebuild kernels behind it): the arrays the skin kernel writes word for word against the host
statement rtx_scene_skinned_prims, the pose's words against rtx_scene_pose_prims_records of those arrays, and every posed
call over such a pose against an ORACLE SCENE CREATED WITH THE STATED PRIMITIVES and against rtx_scene_pose_prims with
those arrays (tests/skin_sets.py, whose conditions tests/test_skin_sets.py asserts without a GPU).  Every comparison is
for equal bits or bytes."""
import importlib

import numpy as np
import pytest

import moves_sets as mv
import prims_sets as pm
import query_sets as qs
import shade_sets as ss
import skin_sets as sk
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
    """one yard for the module: every test binds the skin it needs"""
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
    """the pose's arrays on the device -> (keywords of rtx.Scene.pose_skinned_device, the tensors that keep them alive);
    guard: so many trailing NaN entries behind moves and radius_scale"""
    keep = {}
    for k in ("moves", "radius_scale", "rgb", "sphere_rgb"):
        a = kw.get(k)
        if a is None:
            continue
        a = np.ascontiguousarray(a)
        if guard and k in ("moves", "radius_scale"):
            a = np.concatenate([a, np.full((guard,) + a.shape[1:], np.nan, F)])
        keep[k] = torch.from_numpy(a).to("cuda:0")
    torch.cuda.synchronize()
    names = dict(moves="d_moves_ptr", radius_scale="d_radius_scale_ptr", rgb="d_rgb_ptr", sphere_rgb="d_sphere_rgb_ptr")
    out = {names[k]: t.data_ptr() for k, t in keep.items()}
    out["n_moves"] = len(kw["moves"])
    return out, keep


# ---------------------------------------------------------------------------------------------- 1: the device's arrays
@pytest.mark.parametrize("name", sk.POSES)
def test_the_devices_arrays_and_the_pose_are_the_host_statements_on_the_yard(rtx, samples_seeded, yard, name):
    torch = pytest.importorskip("torch")
    kw = sk.moves(rtx, name)
    yard.skin(**sk.skin(rtx, name))
    want = yard.skinned_prims(**sk.statement_kw(kw))
    stated = sk.stated(rtx, samples_seeded, name)
    assert np.array_equal(bits(want[0]), bits(stated["tris"])) and np.array_equal(bits(want[1]), bits(stated["spheres"]))
    given = sk.given(rtx, samples_seeded, name)
    rank = np.arange(pm.N_PRIMS, dtype=np.uint32)[::-1].copy()
    d_rank = torch.from_numpy(rank.view(np.int32)).to("cuda:0")
    dkw, keep = on_device(torch, kw)
    stream = torch.cuda.current_stream().cuda_stream
    for rebuilt in (False, True):
        st = yard.pose_skinned(rebuilt=rebuilt, stats=True, **kw)
        assert st["kernel_ms"] > 0 and st["rays"] == 0
        same_arrays(yard.debug_moved_prims(), want, name + ", host variant")
        check_pose(yard, given, name + ", host variant", rebuilt)
        yard.pose_skinned(rebuilt=rebuilt, tie_rank=rank, **kw)
        check_pose(yard, given, name + ", host variant, given ranks", rebuilt, tie_rank=rank)
        yard.pose(pm.yard(rtx)["tris"])                                 # (a host pose between: the buffers are reused)
        yard.pose_skinned_device(0, rebuilt=rebuilt, stream=stream, **dkw)
        same_arrays(yard.debug_moved_prims(), want, name + ", device variant")
        check_pose(yard, given, name + ", device variant", rebuilt)
        yard.pose_skinned_device(0, rebuilt=rebuilt, stream=stream, d_tie_rank_ptr=d_rank.data_ptr(), **dkw)
        check_pose(yard, given, name + ", device variant, given ranks", rebuilt, tie_rank=rank)
    torch.cuda.synchronize()


def test_the_devices_arrays_on_the_count_scenes_and_the_smallest(rtx, samples_seeded):
    """255, 256 and 257 primitives, every third a sphere (a workgroup of the skin kernel ends inside a triangle, and at the
    hand-over from corners to spheres), `many`: 257 moves, and 63 / 66 / 255 / 258 corners without a sphere"""
    torch = pytest.importorskip("torch")
    stream = torch.cuda.current_stream().cuda_stream
    cases = [(name, pm.open_sized(rtx, samples_seeded, sc), skin, kw) for name, sc, skin, kw in sk.count_cases(rtx)]
    cases += [(name, sk.open_tris(rtx, samples_seeded, tris), skin, kw) for name, tris, skin, kw in sk.smallest_cases(rtx)]
    for name, opened, skin, kw in cases:
        with opened as scene:
            scene.skin(**skin)
            with pytest.raises(rtx.RtxError) as e:                      # neither kernel ever ran on this scene
                scene.debug_moved_prims()
            assert e.value.code == rtx.ERR_BAD_ARG
            want = scene.skinned_prims(**kw)
            given = dict(v0v1v2=want[0], spheres=want[1] if len(want[1]) else None, rgb=None, sphere_rgb=None)
            dkw, keep = on_device(torch, kw)
            for rebuilt in (False, True):
                scene.pose_skinned(rebuilt=rebuilt, **kw)
                same_arrays(scene.debug_moved_prims(), want, "%s, host variant" % name)
                check_pose(scene, given, "%s, host variant" % name, rebuilt)
                scene.pose_skinned_device(0, rebuilt=rebuilt, stream=stream, **dkw)
                same_arrays(scene.debug_moved_prims(), want, "%s, device variant" % name)
                check_pose(scene, given, "%s, device variant" % name, rebuilt)
            torch.cuda.synchronize()


def test_out_of_range_bones_read_no_move(rtx, samples_seeded, yard):
    """the device variant's preconditions broken: bones of n_moves, n_moves + 1, 0xFFFFFFFE and 65,536 in the skin, fewer
    moves than the bind's largest bone.  Eight NaN entries stand behind the device's moves and radius_scale, so an index
    that was not compared against n_moves shows as NaN words, never as a read out of bounds; the arrays are the host
    statement's, which takes such a bone as RTX_MOVE_NONE"""
    torch = pytest.importorskip("torch")
    stream = torch.cuda.current_stream().cuda_stream
    for name in ("all", "four"):
        kw = sk.moves(rtx, name)
        n_moves = len(kw["moves"])
        skin = sk.skin(rtx, name)
        bones = skin["bones"].copy().reshape(-1, 4)
        wild = np.array([n_moves, n_moves + 1, 0xFFFFFFFE, 65536], np.uint32)
        for k, corner in enumerate((0, 1, 5, 30, 62, 63, 64, 100, 122)):
            bones[corner, k % 4] = wild[k % 4]                          # one slot of a followed corner
        bones[7] = wild                                                 # a corner of nothing but wild bones
        sphere_bone = None if skin["sphere_bone"] is None else skin["sphere_bone"].copy()
        if sphere_bone is not None:
            sphere_bone[[1, 4]] = (n_moves, 0xFFFFFFFE)
        yard.skin(bones.reshape(-1, 3, 4), skin["weights"], sphere_bone)
        assert yard.skin_bound() == (True, 0xFFFFFFFE)
        with pytest.raises(rtx.RtxError) as e:                          # the host variant refuses: n_moves <= max_bone
            yard.pose_skinned(**kw)
        assert e.value.code == rtx.ERR_BAD_ARG
        want = yard.skinned_prims(**sk.statement_kw(kw))
        as_none = np.where(bones >= n_moves, sk.NONE, bones).astype(np.uint32)
        y = pm.yard(rtx)
        restated = sk.restated(y["tris"], y["spheres"], as_none, skin["weights"],
                               None if sphere_bone is None else np.where(sphere_bone >= n_moves, sk.NONE, sphere_bone),
                               kw["moves"], kw["radius_scale"])
        same_arrays(want, restated, name + ": the host statement with wild bones")
        assert np.array_equal(bits(want[0].reshape(-1, 3)[7]), bits(y["tris"].reshape(-1, 3)[7]))
        dkw, keep = on_device(torch, kw, guard=8)
        for rebuilt in (False, True):
            yard.pose_skinned_device(0, rebuilt=rebuilt, stream=stream, **dkw)
            v = np.full(41 * 9 + 16, 7.5, F)
            s = np.full(5 * 4 + 16, 7.5, F)
            f32p = rtx.rtx.f32p
            assert rtx.rtx._lib.rtx_debug_moved_prims(yard.handle, 0, v.ctypes.data_as(f32p), s.ctypes.data_as(f32p)) == rtx.OK
            assert (v[41 * 9:] == 7.5).all() and (s[5 * 4:] == 7.5).all()
            got = v[:41 * 9].reshape(41, 9), s[:20].reshape(5, 4)
            assert np.isfinite(got[0]).all() and np.isfinite(got[1]).all(), name + ": a guard entry was read"
            same_arrays(got, want, name + ", wild bones")
            check_pose(yard, dict(v0v1v2=want[0], spheres=want[1], rgb=kw["rgb"], sphere_rgb=kw["sphere_rgb"]), name + ", wild bones",
                       rebuilt)
        # fewer moves than the skin names: the bones at and above the count are NONE to the kernel as to the statement
        if name == "four":
            yard.skin(**skin)
            short = dict(kw, moves=kw["moves"][:2])
            want = yard.skinned_prims(**sk.statement_kw(short))
            dshort, keep2 = on_device(torch, short, guard=8)
            yard.pose_skinned_device(0, stream=stream, **dshort)
            got = yard.debug_moved_prims()
            assert np.isfinite(got[0]).all()
            same_arrays(got, want, "four with two moves")
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


@pytest.mark.parametrize("name", sk.CALLS)
def test_views_and_rows_are_the_oracle_scene_and_the_prims_pose(rtx, orc, samples_seeded, yard, name):
    p = sk.posed(orc, rtx, samples_seeded, name)
    kw = sk.moves(rtx, name)
    yard.skin(**sk.skin(rtx, name))
    given = sk.given(rtx, samples_seeded, name)
    tri, count = pm.POSE_LIGHT
    light = rtx.Scene.make_light(tri, count)
    lit, lit_stats = sk.lit_frame(orc, rtx, samples_seeded, name)
    assert (lit != p["frame"]).any()
    results = []
    for rebuilt in (False, True):
        what = "%s, %s" % (name, "rebuilt" if rebuilt else "refitted")
        yard.pose_skinned(rebuilt=rebuilt, **kw)
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


@pytest.mark.parametrize("name", sk.CALLS)
def test_ray_queries_and_shading_over_a_skinned_pose(rtx, orc, samples_seeded, yard, name):
    (ro, rd, exp), (to, tt, texp, occ) = sk.query_set(orc, rtx, samples_seeded, name)
    tb = sk.tables(orc, rtx, samples_seeded, name)
    s = sk.composition(orc, rtx, samples_seeded, name)
    kw = sk.moves(rtx, name)
    yard.skin(**sk.skin(rtx, name))
    given = sk.given(rtx, samples_seeded, name)
    for rebuilt in (False, True):
        got = []
        for skinned in (True, False):
            if skinned:
                yard.pose_skinned(rebuilt=rebuilt, **kw)
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
        assert got[0] == got[1], "%s: a skinned pose and rtx_scene_pose_prims of the stated arrays differ" % name


# ---------------------------------------------------------------------------------------------- 3: the tree rules
def test_hard_rays_onto_the_bent_cluster_follow_the_reference_tree_rule(rtx, orc, samples_seeded, yard):
    o, d, exp, twin = sk.hard_rays(orc, rtx, samples_seeded)
    kw = sk.moves(rtx, "bend")
    yard.skin(**sk.skin(rtx, "bend"))
    (ro, rd, qexp), _ = sk.query_set(orc, rtx, samples_seeded, "bend")
    for rebuilt in (False, True):
        yard.pose_skinned(rebuilt=rebuilt, reference_tree=rtx.REFTREE_ALWAYS, **kw)  # the oracle's own tree over the STATED boxes
        for order in (dict(keep_order=True), dict(force_regroup=True)):
            qs.check_hits(yard.trace_rays(o, d, posed=True, **order), exp, None, "hard rays under RTX_REFTREE_ALWAYS %s" % order)
        qs.check_hits(yard.trace_rays(ro, rd, posed=True), qexp, None, "ordinary rays under RTX_REFTREE_ALWAYS")
        yard.pose_skinned(rebuilt=rebuilt, reference_tree=rtx.REFTREE_NEVER, **kw)
        # RTX_REFTREE_NEVER: the pose's stream with the reference's box test — some tree over these primitives; it
        # terminates, and what it reports is a hit of the ray, so never nearer than the twin's closest one
        got = yard.trace_rays(o, d, posed=True, keep_order=True)
        hit = got["prim"] != NO_HIT
        assert (twin["prim"][hit] != NO_HIT).all() and (got["t"][hit] >= twin["t"][hit]).all()
        assert np.array_equal(got["prim"][hit & (got["t"] == twin["t"])], twin["prim"][hit & (got["t"] == twin["t"])])


def test_an_exact_tie_between_a_sphere_a_skin_brings_and_a_triangle(rtx, orc, samples_seeded):
    o, d = pm.TIE_RAY
    rgb = np.ones((2, 3), F)
    osc = orc.Scene(8, 8, pm.TIE_TRIS, rgb, samples_seeded[:4096], spheres=pm.TIE_MOVED, kinds=pm.TIE_KINDS, **pm.TIE_KW)
    exp, _ = qs.oracle_hits(orc, osc, o, d, qs.HIT_DTYPE)
    osc.close()
    kw = sk.TIE_MOVES
    with rtx.Scene(8, 8, pm.TIE_TRIS, rgb, samples_seeded[:4096], spheres=pm.TIE_SPHERES, kinds=pm.TIE_KINDS, **pm.TIE_KW) as scene:
        scene.skin(**sk.TIE_SKIN)
        v, s = scene.skinned_prims(**kw)
        assert np.array_equal(bits(s), bits(pm.TIE_MOVED)) and np.array_equal(bits(v), bits(pm.TIE_TRIS))
        for rebuilt in (False, True):
            scene.pose_skinned(rebuilt=rebuilt, reference_tree=rtx.REFTREE_ALWAYS, **kw)
            got = scene.trace_rays(o, d, posed=True)
            assert np.array_equal(got["prim"], exp["prim"]) and np.array_equal(bits(got["t"]), bits(exp["t"])), rebuilt
            scene.pose_skinned(rebuilt=rebuilt, reference_tree=rtx.REFTREE_NEVER, **kw)
            assert scene.trace_rays(o, d, posed=True)["prim"][0] == 1          # NULL ranks: the larger index, the sphere
            scene.pose_skinned(rebuilt=rebuilt, tie_rank=np.array([5, 3, 0], np.uint32), **kw)
            assert scene.trace_rays(o, d, posed=True)["prim"][0] == 0          # the larger tie_rank, the triangle
            scene.pose_skinned(rebuilt=rebuilt, tie_rank=np.array([2, 3, 9], np.uint32), reference_tree=rtx.REFTREE_ALWAYS, **kw)
            assert scene.trace_rays(o, d, posed=True)["prim"][0] == 1          # given ranks go before the tree's
            assert scene.trace_rays(o, d)["prim"][0] == 0                      # unposed: the sphere is elsewhere


# ---------------------------------------------------------------------------------------------- 4: state
def test_sequences(rtx, orc, samples_seeded):
    view = lib_view(rtx)
    frames = {n: sk.posed(orc, rtx, samples_seeded, n)["frame"] for n in sk.POSES}
    y = pm.yard(rtx)
    with pm.open_yard(rtx, samples_seeded) as scene, pm.open_yard(rtx, samples_seeded) as other:
        usual = scene.render_rows().tobytes()
        unposed = scene.render_view_rows(view).tobytes(), scene.render_view(view).tobytes()
        # no skin: refused, and nothing is posed
        with pytest.raises(rtx.RtxError) as e:
            scene.pose_skinned(**sk.moves(rtx, "bend"))
        assert e.value.code == rtx.ERR_BAD_ARG
        # skinned -> plain rtx_scene_pose -> skinned, under a standing eye
        scene.skin(**sk.skin(rtx, "all"))
        scene.pose_skinned(**sk.moves(rtx, "all"))
        assert np.array_equal(scene.render_view_rows(view, posed=True), frames["all"])
        bent = sk.stated(rtx, samples_seeded, "bend")["tris"]
        scene.pose(bent)                                            # spheres and colours are the uploaded ones again
        assert np.array_equal(scene.render_view_rows(view, posed=True), frames["bend"])
        with pytest.raises(rtx.RtxError) as e:                      # ... and the skin kernel's arrays are gone
            scene.debug_moved_prims()
        assert e.value.code == rtx.ERR_BAD_ARG
        scene.pose_skinned(rebuilt=True, **sk.moves(rtx, "all"))
        assert np.array_equal(scene.render_view_rows(view, posed=True), frames["all"])
        # a re-bind between two poses: the pose that stands on the device stays until the next pose, which picks it up
        scene.skin(**sk.skin(rtx, "four"))
        assert np.array_equal(scene.render_view_rows(view, posed=True), frames["all"])
        assert np.array_equal(scene.render_view(view, posed=True), frames["all"])
        all_ = sk.stated(rtx, samples_seeded, "all")
        same_arrays(scene.debug_moved_prims(), (all_["tris"], all_["spheres"]), "after a re-bind")
        scene.pose_skinned(**sk.moves(rtx, "four"))
        assert np.array_equal(scene.render_view_rows(view, posed=True), frames["four"])
        four = sk.stated(rtx, samples_seeded, "four")
        same_arrays(scene.debug_moved_prims(), (four["tris"], four["spheres"]), "after the re-bound pose")
        # a moved pose between two skinned ones: its kernel and the skin kernel write the same two buffers
        scene.pose_moved(**mv.moves(rtx, "turn"))
        assert np.array_equal(scene.render_view_rows(view, posed=True), mv.posed(orc, rtx, samples_seeded, "turn")["frame"])
        scene.pose_skinned(rebuilt=True, **sk.moves(rtx, "four"))
        assert np.array_equal(scene.render_view_rows(view, posed=True), frames["four"])
        # a refused skinned pose leaves the previous pose standing
        with pytest.raises(rtx.RtxError) as e:
            scene.pose_skinned(**dict(sk.moves(rtx, "four"), moves=sk.four_moves(rtx)[:3]))      # n_moves <= max_bone
        assert e.value.code == rtx.ERR_BAD_ARG
        wild = sk.four_moves(rtx)
        wild[2, 3] = 1e6
        with pytest.raises(rtx.RtxError) as e:
            scene.pose_skinned(moves=wild)
        assert e.value.code == rtx.ERR_UNSUPPORTED
        assert np.array_equal(scene.render_view_rows(view, posed=True), frames["four"])
        same_arrays(scene.debug_moved_prims(), (four["tris"], four["spheres"]), "after a refused pose")
        # unbound: refused again; the pose still stands
        scene.skin()
        with pytest.raises(rtx.RtxError) as e:
            scene.pose_skinned(**sk.moves(rtx, "four"))
        assert e.value.code == rtx.ERR_BAD_ARG
        assert np.array_equal(scene.render_view_rows(view, posed=True), frames["four"])
        # `rest` equals the unposed calls, and rtx_scene_pose of the created vertices
        scene.skin(**sk.skin(rtx, "rest"))
        scene.pose_skinned(**sk.moves(rtx, "rest"))
        assert (scene.render_view_rows(view, posed=True).tobytes(), scene.render_view(view, posed=True).tobytes()) == unposed
        skinned = scene.debug_pose()
        scene.pose(y["tris"])
        same_words(skinned, scene.debug_pose(), "`rest` against rtx_scene_pose of the created vertices")
        # two live scenes, each its own skin and pose
        scene.skin(**sk.skin(rtx, "lean"))
        other.skin(**sk.skin(rtx, "bend"))
        scene.pose_skinned(**sk.moves(rtx, "lean"))
        other.pose_skinned(rebuilt=True, **sk.moves(rtx, "bend"))
        for k in range(2):
            assert np.array_equal(scene.render_view_rows(view, posed=True), frames["lean"])
            assert np.array_equal(other.render_view_rows(view, posed=True), frames["bend"])
        # the unposed calls give the scene's usual bytes
        assert scene.render_rows().tobytes() == usual and other.render_rows().tobytes() == usual
        assert (scene.render_view_rows(view).tobytes(), scene.render_view(view).tobytes()) == unposed


def test_many_moves_on_their_scene(rtx, orc, samples_seeded):
    """257 moves on the 257-primitive scene: the frame against the oracle scene created with the stated primitives"""
    name, sc, skin, kw = sk.count_cases(rtx)[-1]
    assert name == "many"
    cam = dict(eye=(0.0, 100.0, 200.0), look_at=(-15.0, 100.0, 0.0), up=vs.UP, distance=30.0)
    view = rtx.Scene.view(24, 16, **cam)
    with pm.open_sized(rtx, samples_seeded, sc) as scene:
        scene.skin(**skin)
        v, s = scene.skinned_prims(**kw)
        osc = orc.Scene(24, 16, v, sc["rgb"], samples_seeded[:4096], spheres=s, sphere_rgb=sc["sphere_rgb"], kinds=sc["kinds"],
                        nb_ray=1, nb_light_sample=4, **cam)
        want, _ = osc.render_rows(mode=orc.MODE_BVH)
        osc.close()
        usual = scene.render_rows().tobytes()
        still = scene.render_view(view)
        for rebuilt in (False, True):
            scene.pose_skinned(rebuilt=rebuilt, **kw)
            assert np.array_equal(scene.render_view(view, posed=True), want), where(scene.render_view(view, posed=True), want)
            assert np.array_equal(scene.render_view_rows(view, posed=True), want)
        assert (want != still).any() and (want != want[0, 0]).any()
        assert scene.render_rows().tobytes() == usual and np.array_equal(scene.render_view(view), still)


# ---------------------------------------------------------------------------------------------- 5: device-resident, frames
def test_device_resident_skinned_poses_and_posed_rows_on_one_stream(rtx, orc, samples_seeded):
    torch = pytest.importorskip("torch")
    assert torch.cuda.is_available(), "torch sees no GPU"
    view = lib_view(rtx)
    n = view.ny * view.width * 3
    frames = [sk.posed(orc, rtx, samples_seeded, k)["frame"] for k in ("bend", "all", "balls")]
    stream = torch.cuda.Stream(device="cuda:0")
    assert stream.cuda_stream != torch.cuda.default_stream().cuda_stream
    with sk.open_skinned(rtx, samples_seeded, "all") as scene, torch.cuda.stream(stream):
        on = [on_device(torch, sk.moves(rtx, k)) for k in ("bend", "all")]      # `all`'s skin is `bend`'s with sphere bones:
        on[0][0]["n_moves"] = 7                                                  # `bend` as `all`'s skin over `bend`'s two moves
        bend_then_rest = np.concatenate([sk.bend_moves(rtx), np.tile(mv.IDENTITY, (5, 1))]).astype(F)
        d_bend = torch.from_numpy(bend_then_rest).to("cuda:0")
        on[0][0]["d_moves_ptr"] = d_bend.data_ptr()
        bufs = [torch.full((n + 16,), 0xAA, dtype=torch.uint8, device="cuda:0") for _ in range(3)]
        stream.synchronize()
        want_first = scene.skinned_prims(bend_then_rest)
        # a refitted skinned pose, its rows, a rebuilt one, its rows twice: one stream, nothing waited for
        scene.pose_skinned_device(0, stream=stream.cuda_stream, **on[0][0])
        scene.render_view_rows_device(0, view, bufs[0].data_ptr(), bufs[0].numel(), stream.cuda_stream, posed=True)
        scene.pose_skinned_device(0, rebuilt=True, stream=stream.cuda_stream, **on[1][0])
        scene.render_view_rows_device(0, view, bufs[1].data_ptr(), bufs[1].numel(), stream.cuda_stream, posed=True)
        scene.render_view_rows_device(0, view, bufs[2].data_ptr(), bufs[2].numel(), stream.cuda_stream, posed=True)
        # ... and a host posed call right behind them, on the library's stream: it waits for the event
        assert np.array_equal(scene.render_view_rows(view, posed=True), frames[1])
        # ... and a re-bind and a host skinned pose: the upload waits for the launches that still read the skin it replaces
        scene.skin(**sk.skin(rtx, "balls"))
        scene.pose_skinned(**sk.moves(rtx, "balls"))
        stream.synchronize()
        # identity moves under the spheres' bones leave x + 0 = x: `bend`'s triangles, the spheres as created
        bend = sk.stated(rtx, samples_seeded, "bend")
        assert np.array_equal(bits(want_first[0]), bits(bend["tris"])) and np.array_equal(want_first[1], pm.SPHERES)
        for f, b in zip((frames[0], frames[1], frames[1]), bufs):
            out = b.cpu().numpy()
            assert out[:n].tobytes() == f.tobytes() and (out[n:] == 0xAA).all()
        assert np.array_equal(scene.render_view_rows(view, posed=True), frames[2])


def test_four_frames_of_a_bend(rtx, orc, samples_seeded, yard):
    """a bend in four steps, 96 bytes each; every frame against the oracle scene created with the stated vertices"""
    view = lib_view(rtx)
    yard.skin(**sk.skin(rtx, "bend"))
    c = mv.cluster_centre(rtx)
    seen = []
    for k, degrees in enumerate((25.0, 50.0, 75.0, 100.0)):
        a = np.deg2rad(degrees)
        m = np.stack([mv.IDENTITY, mv.about([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]], c)]).astype(F)
        v, s = yard.skinned_prims(m)
        prims = dict(pm.yard_pose(rtx, "identity"), tris=v, spheres=s)
        r = pm.render(orc, samples_seeded, prims)
        r["osc"].close()
        yard.pose_skinned(m, rebuilt=bool(k % 2))
        got = yard.render_view_rows(view, posed=True)
        assert np.array_equal(got, r["frame"]), "frame %d differs from the oracle scene at %s" % (k, where(got, r["frame"]))
        assert np.array_equal(yard.render_view(view, posed=True), r["frame"])
        seen.append(got.tobytes())
    assert len(set(seen)) >= 3
