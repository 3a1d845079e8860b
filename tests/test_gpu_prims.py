"""GPU parity of a pose that states every field of a primitive (rtx_scene_pose_prims, rtx_scene_pose_prims_device: the
overlay kernel and the pose or rebuild kernels behind it): the device's records, node words, plane records and aimed stream
word for word against the host statement, and every posed call over such a pose against an ORACLE SCENE CREATED WITH THE
POSED PRIMITIVES (tests/prims_sets.py, whose conditions tests/test_prims_sets.py asserts without a GPU).  Every comparison
is for equal bits or bytes."""
import importlib

import numpy as np
import pytest

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


def lib_view(rtx, v=pm.YARD_VIEW):
    (w, h) = v[0]
    return rtx.Scene.view(w, h, **vs.camera(v))


def where(got, want):
    return np.argwhere((got != want).any(axis=2))[:8].tolist()


def same_words(got, want, what):
    for g, w, part in zip(got, want, ("primitive", "shading", "node", "aimed", "permutation")):
        if w is None:
            continue
        bad = np.argwhere(g != w)
        assert not len(bad), "%s: %s words differ at %s" % (what, part, bad[:6].tolist())


def check_device(scene, given, what, rebuilt, eye=pm.YARD_VIEW[1], tie_rank=None):
    """the pose the device holds against rtx_scene_pose_prims_records / _aimed, read back by rtx_debug_pose and
    rtx_debug_pose_pipeline, or by rtx_debug_pose_rebuilt"""
    aimed = scene.pose_prims_aimed(eye, rebuilt=rebuilt, **given)
    if rebuilt:
        keys, perm, t, s, n = scene.pose_prims_records(rebuilt=True, tie_rank=tie_rank, **given)
        dperm, dt, ds, dn, daimed = scene.debug_pose_rebuilt(eye=eye)
        same_words((dt, ds, dn, daimed, dperm), (t, s, n, aimed, perm), what + ", rebuilt")
    else:
        t, s, n = scene.pose_prims_records(tie_rank=tie_rank, **given)
        dt, ds, dn = scene.debug_pose()
        planes, daimed = scene.debug_pose_pipeline(eye=eye)
        same_words((dt, ds, dn, daimed), (t, s, n, aimed), what + ", refitted")
        v = scene.tris if given.get("v0v1v2") is None else given["v0v1v2"]
        if len(v):
            assert np.array_equal(planes, scene.posed_pipeline_records(v)[0]), what + ": plane records"


def on_device(torch, given):
    """the pose's arrays on the device -> (keywords of rtx.Scene.pose_prims_device, the tensors that keep them alive)"""
    keep = {k: torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0") for k, a in given.items() if a is not None and len(a)}
    torch.cuda.synchronize()
    names = dict(v0v1v2="d_v0v1v2_ptr", spheres="d_spheres_ptr", rgb="d_rgb_ptr", sphere_rgb="d_sphere_rgb_ptr")
    kw = {names[k]: t.data_ptr() for k, t in keep.items()}
    kw.setdefault("d_v0v1v2_ptr", None)
    return kw, keep


# ---------------------------------------------------------------------------------------------- 1: the words
@pytest.mark.parametrize("name", pm.POSES)
def test_device_words_are_the_hosts_on_the_yard(rtx, yard, name):
    torch = pytest.importorskip("torch")
    given = pm.given(rtx, name)
    rank = np.arange(pm.N_PRIMS, dtype=np.uint32)[::-1].copy()
    d_rank = torch.from_numpy(rank.view(np.int32)).to("cuda:0")
    kw, keep = on_device(torch, given)
    stream = torch.cuda.current_stream().cuda_stream
    for rebuilt in (False, True):
        st = yard.pose_prims(rebuilt=rebuilt, stats=True, **given)
        assert st["kernel_ms"] > 0 and st["rays"] == 0
        check_device(yard, given, name + ", host variant", rebuilt)
        yard.pose_prims(rebuilt=rebuilt, tie_rank=rank, **given)
        check_device(yard, given, name + ", host variant, given ranks", rebuilt, tie_rank=rank)
        yard.pose_prims_device(0, rebuilt=rebuilt, stream=stream, **kw)
        check_device(yard, given, name + ", device variant", rebuilt)
        yard.pose_prims_device(0, rebuilt=rebuilt, stream=stream, d_tie_rank_ptr=d_rank.data_ptr(), **kw)
        check_device(yard, given, name + ", device variant, given ranks", rebuilt, tie_rank=rank)
    torch.cuda.synchronize()


def test_device_words_are_the_hosts_on_the_sizes_at_which_indexing_can_go_wrong(rtx, samples_seeded):
    torch = pytest.importorskip("torch")
    stream = torch.cuda.current_stream().cuda_stream
    for name, sc in pm.size_scenes(rtx).items():
        with pm.open_sized(rtx, samples_seeded, sc) as scene:
            full = pm.pose_kw(sc["pose"])
            own = dict(v0v1v2=sc["tris"], spheres=sc["spheres"], rgb=sc["rgb"], sphere_rgb=sc["sphere_rgb"])
            for given, what in ((full, "posed"), (own, "identity"), (dict(full, rgb=None, sphere_rgb=None), "spheres alone"),
                                (dict(own, spheres=None), "colours alone"), (full, "posed again")):
                given = {k: (a if a is None or len(a) else None) for k, a in given.items()}
                kw, keep = on_device(torch, given)
                for rebuilt in (False, True):
                    scene.pose_prims(rebuilt=rebuilt, **given)
                    check_device(scene, given, "%s %s, host variant" % (name, what), rebuilt)
                    scene.pose_prims_device(0, rebuilt=rebuilt, stream=stream, **kw)
                    check_device(scene, given, "%s %s, device variant" % (name, what), rebuilt)
                torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------- 2: posed frames
@pytest.mark.parametrize("name", pm.POSES)
def test_views_and_rows_are_the_oracle_scene_with_the_posed_primitives(rtx, orc, samples_seeded, yard, name):
    p = pm.posed(orc, rtx, samples_seeded, name)
    view = lib_view(rtx)
    frames = []
    for rebuilt in (False, True):
        yard.pose_prims(rebuilt=rebuilt, **pm.given(rtx, name))
        rgb, shade, hits, st = yard.render_view(view, stats=True, want_shade=True, want_hits=True, posed=True)
        what = "%s, %s" % (name, "rebuilt" if rebuilt else "refitted")
        assert np.array_equal(rgb, p["frame"]), "%s: bytes differ from the oracle scene at (y, x) %s" % (what, where(rgb, p["frame"]))
        assert np.array_equal(bits(shade["linear"]), bits(p["lin"])), what + ": linear differs from the oracle scene's"
        assert np.array_equal(shade["rgb8"], rgb), what
        assert np.array_equal(hits["prim"][:, :, 0], p["tri"]), what + ": hit primitives differ"
        assert st["primary_hits"] == p["stats"]["primary_hits"] and st["shadow_rays"] == p["stats"]["shadow_rays"], (what, st)
        rows, rst = yard.render_view_rows(view, stats=True, posed=True)
        assert np.array_equal(rows, p["frame"]), "%s: rows differ from the oracle scene at (y, x) %s" % (what, where(rows, p["frame"]))
        assert rst["primary_hits"] == p["stats"]["primary_hits"] and rst["shadow_rays"] == p["stats"]["shadow_rays"]
        assert np.array_equal(yard.render_view_rows(view, posed=True), rows)              # the aimed stream standing
        frames.append((rgb, shade.tobytes(), hits.tobytes(), rows))
    assert all(np.array_equal(a, b) if isinstance(a, np.ndarray) else a == b for a, b in zip(*frames)), name + ": refitted and rebuilt differ"


@pytest.mark.parametrize("name", ["move", "all"])
def test_ray_queries_and_shading_on_the_posed_primitives(rtx, orc, samples_seeded, yard, name):
    (ro, rd, exp), (to, tt, texp, occ) = pm.query_set(orc, rtx, samples_seeded, name)
    tb = pm.tables(orc, rtx, name)
    s = pm.composition(orc, rtx, samples_seeded, name)
    for rebuilt in (False, True):
        yard.pose_prims(rebuilt=rebuilt, **pm.given(rtx, name))
        for n in (1, 64, 65, len(ro)):
            for kw in (dict(keep_order=True), dict(force_regroup=True), dict()):
                got = yard.trace_rays(ro[:n], rd[:n], posed=True, **kw)
                qs.check_hits(got, exp[:n], None, "%s trace %d %s" % (name, n, kw))
                qs.check_normals(got, exp[:n], tb["normals"], pm.kinds(), "%s trace %d %s" % (name, n, kw))
                got = yard.occluded_rays(to[:n], tt[:n], posed=True, **kw)
                assert np.array_equal(got, occ[:n]), (name, n, kw, np.nonzero(got != occ[:n])[0][:8])
        for n0, n in ((0, 64), (100, 65), (250, 127)):          # pixels of the yard view: render_pixel for a batch
            part = ss.take(s, np.arange(n0, n0 + n))
            for kw in (dict(keep_order=True), dict(force_regroup=True)):
                shade, hits = yard.shade_rays(part["origins"], part["directions"], want_hits=True, posed=True, **kw)
                assert shade.tobytes() == part["shade"].tobytes(), (name, n0, n, kw)
                assert hits.tobytes() == yard.trace_rays(part["origins"], part["directions"], keep_order=True, posed=True).tobytes()


def test_a_pose_under_a_given_light(rtx, orc, samples_seeded, yard):
    tri, count = pm.POSE_LIGHT
    light = rtx.Scene.make_light(tri, count)
    frame, ost = pm.lit_frame(orc, rtx, samples_seeded, "all")
    view = lib_view(rtx)
    own = pm.posed(orc, rtx, samples_seeded, "all")["frame"]
    assert (frame != own).any()
    for rebuilt in (False, True):
        yard.pose_prims(rebuilt=rebuilt, **pm.given(rtx, "all"))
        lit = yard.render_view(view, stats=True, posed=True, light=light)
        assert np.array_equal(lit[0], frame), "lit posed view differs from the oracle scene at %s" % where(lit[0], frame)
        assert lit[1]["shadow_rays"] == ost["shadow_rays"]
        rows = yard.render_view_rows(view, posed=True, light=light)
        assert np.array_equal(rows, frame), "lit posed rows differ from the oracle scene at %s" % where(rows, frame)
        assert np.array_equal(yard.render_view_rows(view, posed=True), own)             # the scene's light afterwards


# ---------------------------------------------------------------------------------------------- 3: the tree rules
def test_hard_rays_onto_a_moved_sphere_follow_the_reference_tree_rule(rtx, orc, samples_seeded, yard):
    o, d, exp, twin = pm.hard_rays(orc, rtx, samples_seeded)
    given = pm.given(rtx, "move")
    (ro, rd, qexp), _ = pm.query_set(orc, rtx, samples_seeded, "move")
    for rebuilt in (False, True):
        yard.pose_prims(rebuilt=rebuilt, reference_tree=rtx.REFTREE_ALWAYS, **given)   # the oracle's own tree over the POSED boxes
        for kw in (dict(keep_order=True), dict(force_regroup=True)):
            qs.check_hits(yard.trace_rays(o, d, posed=True, **kw), exp, None, "hard rays under RTX_REFTREE_ALWAYS %s" % kw)
        qs.check_hits(yard.trace_rays(ro, rd, posed=True), qexp, None, "ordinary rays under RTX_REFTREE_ALWAYS")
        # RTX_REFTREE_NEVER: the pose's stream with the reference's box test — some tree over these primitives; it
        # terminates, and every hit it reports is the twin's or a miss
        yard.pose_prims(rebuilt=rebuilt, reference_tree=rtx.REFTREE_NEVER, **given)
        got = yard.trace_rays(o, d, posed=True, keep_order=True)
        hit = got["prim"] != NO_HIT
        assert np.array_equal(got["prim"][hit], twin["prim"][hit])


def test_an_exact_tie_between_a_moved_sphere_and_a_triangle(rtx, orc, samples_seeded):
    o, d = pm.TIE_RAY
    rgb = np.ones((2, 3), F)
    osc = orc.Scene(8, 8, pm.TIE_TRIS, rgb, samples_seeded[:4096], spheres=pm.TIE_MOVED, kinds=pm.TIE_KINDS, **pm.TIE_KW)
    exp, _ = qs.oracle_hits(orc, osc, o, d, qs.HIT_DTYPE)
    osc.close()
    with rtx.Scene(8, 8, pm.TIE_TRIS, rgb, samples_seeded[:4096], spheres=pm.TIE_SPHERES, kinds=pm.TIE_KINDS, **pm.TIE_KW) as scene:
        for rebuilt in (False, True):
            scene.pose_prims(spheres=pm.TIE_MOVED, rebuilt=rebuilt, reference_tree=rtx.REFTREE_ALWAYS)
            got = scene.trace_rays(o, d, posed=True)
            assert np.array_equal(got["prim"], exp["prim"]) and np.array_equal(bits(got["t"]), bits(exp["t"])), rebuilt
            scene.pose_prims(spheres=pm.TIE_MOVED, rebuilt=rebuilt, reference_tree=rtx.REFTREE_NEVER)
            assert scene.trace_rays(o, d, posed=True)["prim"][0] == 1          # NULL ranks: the larger index, the sphere
            scene.pose_prims(spheres=pm.TIE_MOVED, rebuilt=rebuilt, tie_rank=np.array([5, 3, 0], np.uint32))
            assert scene.trace_rays(o, d, posed=True)["prim"][0] == 0          # the larger tie_rank, the triangle
            scene.pose_prims(spheres=pm.TIE_MOVED, rebuilt=rebuilt, tie_rank=np.array([2, 3, 9], np.uint32), reference_tree=rtx.REFTREE_ALWAYS)
            assert scene.trace_rays(o, d, posed=True)["prim"][0] == 1          # given ranks go before the tree's
            assert scene.trace_rays(o, d)["prim"][0] == 0                      # unposed: the sphere is elsewhere


# ---------------------------------------------------------------------------------------------- 4: sequences
def test_sequences(rtx, orc, samples_seeded):
    view = lib_view(rtx)
    frames = {n: pm.posed(orc, rtx, samples_seeded, n)["frame"] for n in pm.POSES}
    y = pm.yard(rtx)
    turned = pm.yard_pose(rtx, "all")["tris"]
    with pm.open_yard(rtx, samples_seeded) as scene, pm.open_yard(rtx, samples_seeded) as other:
        usual = scene.render_rows().tobytes()
        unposed = scene.render_view_rows(view).tobytes(), scene.render_view(view).tobytes()
        assert np.array_equal(scene.render_view_rows(view), frames["identity"])
        # identity equals rtx_scene_pose byte for byte: the words and the frames
        scene.pose(y["tris"])
        plain = scene.debug_pose(), scene.render_view_rows(view, posed=True), scene.render_view(view, posed=True)
        scene.pose_prims(**pm.given(rtx, "identity"))
        same_words(scene.debug_pose(), plain[0], "identity against rtx_scene_pose")
        assert np.array_equal(scene.render_view_rows(view, posed=True), plain[1]) and np.array_equal(scene.render_view(view, posed=True), plain[2])
        # a prims pose, then a plain pose of the same vertices: spheres and colours are the uploaded ones again
        for make_prims, make_plain in ((False, scene.pose), (True, scene.pose_rebuilt), (False, scene.pose_rebuilt)):
            scene.pose_prims(rebuilt=make_prims, **pm.given(rtx, "all"))
            assert np.array_equal(scene.render_view_rows(view, posed=True), frames["all"])
            make_plain(turned)
            t, s, _ = scene.posed_records(turned)
            got = scene.debug_pose_rebuilt()[1:3] if make_plain == scene.pose_rebuilt else scene.debug_pose()[:2]
            by_idx = lambda a: a[np.argsort(a[:, 15])]
            assert np.array_equal(by_idx(got[0]), by_idx(t)) and np.array_equal(got[1], s), "a plain pose kept part of the prims pose"
            plain_frame = scene.render_view_rows(view, posed=True)
            assert (plain_frame != frames["all"]).any()
            assert scene.render_view_rows(view).tobytes() == unposed[0], "the unposed rows changed"
        # NULL is "as uploaded", never "as the previous pose": recolour after move shows the uploaded spheres
        scene.pose_prims(**pm.given(rtx, "move"))
        assert np.array_equal(scene.render_view(view, posed=True), frames["move"])
        scene.pose_prims(**pm.given(rtx, "recolour"))
        assert np.array_equal(scene.render_view(view, posed=True), frames["recolour"])
        assert np.array_equal(scene.render_view_rows(view, posed=True), frames["recolour"])
        # a refused pose leaves the standing one
        bad = pm.given(rtx, "move")
        bad["spheres"] = bad["spheres"].copy()
        bad["spheres"][1, 0] = 9995.0                             # a box word beyond M
        with pytest.raises(rtx.RtxError) as e:
            scene.pose_prims(**bad)
        assert e.value.code == rtx.ERR_UNSUPPORTED
        assert np.array_equal(scene.render_view_rows(view, posed=True), frames["recolour"])
        check_device(scene, pm.given(rtx, "recolour"), "after a refused pose", False)
        # two live scenes, each its own pose
        other.pose_prims(rebuilt=True, **pm.given(rtx, "radius"))
        for k in range(2):
            assert np.array_equal(scene.render_view_rows(view, posed=True), frames["recolour"])
            assert np.array_equal(other.render_view_rows(view, posed=True), frames["radius"])
        # the unposed calls give the scene's usual bytes
        assert scene.render_rows().tobytes() == usual and other.render_rows().tobytes() == usual
        assert (scene.render_view_rows(view).tobytes(), scene.render_view(view).tobytes()) == unposed


def test_device_resident_prims_pose_and_posed_rows_on_one_stream(rtx, orc, samples_seeded, yard):
    torch = pytest.importorskip("torch")
    assert torch.cuda.is_available(), "torch sees no GPU"
    view = lib_view(rtx)
    n = view.ny * view.width * 3
    names = ("move", "all", "recolour")
    frames = [pm.posed(orc, rtx, samples_seeded, k)["frame"] for k in names]
    stream = torch.cuda.Stream(device="cuda:0")
    assert stream.cuda_stream != torch.cuda.default_stream().cuda_stream
    with torch.cuda.stream(stream):
        on = [on_device(torch, pm.given(rtx, k)) for k in names]
        bufs = [torch.full((n + 16,), 0xAA, dtype=torch.uint8, device="cuda:0") for _ in range(4)]
        stream.synchronize()
        # a refitted prims pose, its rows, a rebuilt one, its view, a refitted one, its rows twice: one stream, nothing waited for
        yard.pose_prims_device(0, stream=stream.cuda_stream, **on[0][0])
        yard.render_view_rows_device(0, view, bufs[0].data_ptr(), bufs[0].numel(), stream.cuda_stream, posed=True)
        yard.pose_prims_device(0, rebuilt=True, stream=stream.cuda_stream, **on[1][0])
        yard.render_view_device(0, view, bufs[1].data_ptr(), None, None, stream.cuda_stream, posed=True)
        yard.pose_prims_device(0, stream=stream.cuda_stream, **on[2][0])
        yard.render_view_rows_device(0, view, bufs[2].data_ptr(), bufs[2].numel(), stream.cuda_stream, posed=True)
        yard.render_view_rows_device(0, view, bufs[3].data_ptr(), bufs[3].numel(), stream.cuda_stream, posed=True)
        # ... and a host posed call right behind them, on the library's stream: it waits for the event
        host = yard.render_view_rows(view, posed=True)
        assert np.array_equal(host, frames[2])
        # ... and a host prims pose: it waits for the launches that still read the pose it replaces
        yard.pose_prims(**pm.given(rtx, "radius"))
        stream.synchronize()
        for f, b in zip((frames[0], frames[1], frames[2], frames[2]), bufs):
            out = b.cpu().numpy()
            assert out[:n].tobytes() == f.tobytes() and (out[n:] == 0xAA).all()
    assert np.array_equal(yard.render_view_rows(view, posed=True), pm.posed(orc, rtx, samples_seeded, "radius")["frame"])


# ---------------------------------------------------------------------------------------------- 5: one arm only
def test_a_scene_without_spheres_recoloured_and_spheres_alone_moved(rtx, orc, samples_seeded):
    y = pm.yard(rtx)
    p = pm.yard_pose(rtx, "recolour")
    view = lib_view(rtx)
    kw = dict(nb_ray=pm.NB_RAY, nb_light_sample=pm.NB_LIGHT, **vs.camera(pm.YARD_VIEW))
    osc = orc.Scene(24, 16, y["tris"], p["rgb"], samples_seeded[:4096], **kw)
    want, _ = osc.render_rows(mode=orc.MODE_BVH)
    osc.close()
    with rtx.Scene(8, 8, y["tris"], y["rgb"], samples_seeded[:4096], reference_tree=rtx.REFTREE_NEVER, tie_rank=None, **kw) as scene:
        still = scene.render_view_rows(view)
        for rebuilt in (False, True):
            scene.pose_prims(rgb=p["rgb"], rebuilt=rebuilt)                       # only recoloured
            check_device(scene, dict(v0v1v2=None, rgb=p["rgb"]), "triangles only", rebuilt)
            assert np.array_equal(scene.render_view_rows(view, posed=True), want) and np.array_equal(scene.render_view(view, posed=True), want)
        assert (want != still).any() and np.array_equal(scene.render_view_rows(view), still)
    moved = pm.yard_pose(rtx, "all")["spheres"]
    none = np.zeros((0, 9), F), np.zeros((0, 3), F)
    osc = orc.Scene(24, 16, none[0], none[1], samples_seeded[:4096], spheres=moved, sphere_rgb=y["sphere_rgb"], **kw)
    want, _ = osc.render_rows(mode=orc.MODE_BVH)
    osc.close()
    with rtx.Scene(8, 8, none[0], none[1], samples_seeded[:4096], spheres=y["spheres"], sphere_rgb=y["sphere_rgb"],
                   reference_tree=rtx.REFTREE_NEVER, tie_rank=None, **kw) as scene:
        still = scene.render_view_rows(view)
        for rebuilt in (False, True):
            scene.pose_prims(spheres=moved, rebuilt=rebuilt)                      # only moved
            check_device(scene, dict(v0v1v2=None, spheres=moved), "spheres only", rebuilt)
            assert np.array_equal(scene.render_view_rows(view, posed=True), want) and np.array_equal(scene.render_view(view, posed=True), want)
        assert (want != still).any() and np.array_equal(scene.render_view_rows(view), still)
