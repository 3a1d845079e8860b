"""GPU parity where zero-area triangles take part (tests/degenerate_sets.py, whose conditions tests/test_degenerate_sets.py
states without a GPU): collinear triangles that Moeller-Trumbore accepts on a determinant of rounding noise, with a NaN
or a meaningless normal; exactly singular triangles and a zero-radius sphere beside them; a collinear needle among the
global triangles; poses that collapse hundreds of triangles onto one point, fold triangles flat and unfold them again;
lights that are a segment and a point.  Frames, ray queries, shaded rays, the pose kernels' words and the lit calls against
the oracle and the host statements.  Every comparison is for equal bits or bytes, with ONE rule for NaN (same_floats):
both sides NaN, in a word where the oracle itself has a NaN and that belongs to a named field — the normal of a Z, C1 or
C2 triangle, the linear colour of a ray whose oracle hit is such a triangle."""
import importlib

import numpy as np
import pytest

import degenerate_sets as dg
import gpu_forms
import np_ref
import query_sets as qs
from query_sets import F, NO_HIT, bits
from test_gpu_lit_rows import check_walk
from test_gpu_prims import on_device, same_words, where
from test_gpu_probe_split import frame_tiles, rows_of, same_under_every_mode
from test_gpu_trace_rays import occluded_every_way, trace_every_way

pytestmark = pytest.mark.gpu
OPTIONS = (dict(keep_order=True), dict(force_regroup=True), dict())
SIZES = (1, 63, 64, 65, 128)


@pytest.fixture(scope="module")
def rtx():
    mod = importlib.import_module("ray-tracer-rust_amd")
    assert mod.device_count() >= 1, "no HIP device: the product path has no CPU fallback"
    assert mod.rtx.RAY_HIT_DTYPE == qs.HIT_DTYPE
    return mod


@pytest.fixture(scope="module")
def scenes(rtx, orc, samples_seeded):
    """name -> dict(scene = the library's, prims, tables, nan = may a primitive's normal be NaN, per Vec position)"""
    made = {}

    def get(name):
        if name not in made:
            if name == "thicket":
                prims = dg.thicket(orc)
                scene = dg.open_scene(rtx, samples_seeded, prims)
                assert scene.info()["n_global"] == 2 and scene.info()["n_ref_nodes"] != 0
            elif name in ("always", "never"):
                prims = dg.thicket(orc)
                scene = dg.open_scene(rtx, samples_seeded, prims, reference_tree=dict(always=rtx.REFTREE_ALWAYS, never=rtx.REFTREE_NEVER)[name])
            else:
                prims = dg.soup(orc, samples_seeded)
                scene = dg.soup_scene(rtx, samples_seeded, prims, nb_ray=2 if name == "soup2" else 1)
            made[name] = dict(scene=scene, prims=prims, tables=dg.tables_of(orc, prims), nan=dg.nan_prims(prims))
        return made[name]
    yield get
    for m in made.values():
        m["scene"].close()


def check_normals(got, exp, tables, nan, what):
    """a triangle's normal is the stored one — orc_triangle_new's, a C3 triangle's garbage bit for bit, NaN where it has
    NaN —, a sphere's normalize(p_hit - origin)"""
    hit = exp["prim"] != NO_HIT
    sphere = np.zeros(len(exp), bool)
    sphere[hit] = tables["sphere"][exp["prim"][hit]]
    tri = hit & ~sphere
    dg.same_floats(got["normal"][tri], tables["normals"][exp["prim"][tri]], nan[exp["prim"][tri]][:, None], what + ": a triangle's normal")
    p = got["p_hit"][sphere]
    want = np.stack(np_ref._normalize(np_ref._sub(np_ref._v(p), np_ref._v(tables["normals"][exp["prim"][sphere]]))), axis=-1)
    assert np.array_equal(bits(got["normal"][sphere]), bits(want)), what + ": a sphere's normal"


def check_shade(got, hits, s, traced, nan, what):
    """rgb8 bytes equal, linear by the NaN rule, hit records rtx_trace_rays'"""
    exp = s["shade"]
    assert np.array_equal(got["rgb8"], exp["rgb8"]), "%s: rgb8 differs at %s" % (what, np.nonzero((got["rgb8"] != exp["rgb8"]).any(axis=1))[0][:8])
    assert np.array_equal(got["hits"], exp["hits"]), what
    prim = s["hit"]["prim"].reshape(len(exp), -1)
    allowed = ((prim != NO_HIT) & nan[np.where(prim != NO_HIT, prim, 0)]).any(axis=1)
    dg.same_floats(got["linear"], exp["linear"], allowed[:, None], what + ": linear")
    if hits is not None:
        assert hits.tobytes() == traced.tobytes(), what + ": the hit records are not rtx_trace_rays'"


# ---------------------------------------------------------------------------------------------- frames
def test_thicket_frames(rtx, orc, samples_seeded, scenes):
    m = scenes("thicket")
    scene, ref = m["scene"], dg.thicket_frame(orc, samples_seeded)
    img, st = gpu_forms.render_both(scene)
    assert np.array_equal(img, ref["frame"]), "rtx_render_rows differs from the oracle at (y, x) %s" % where(img, ref["frame"])
    assert st["primary_hits"] == ref["stats"]["primary_hits"] and st["shadow_rays"] == ref["stats"]["shadow_rays"], st
    view = scene.own_view()
    hit = ref["tri"] != NO_HIT
    allowed = hit & m["nan"][np.where(hit, ref["tri"], 0)]
    for stats in (True, False):
        res = scene.render_view(view, stats=stats, want_shade=True, want_hits=True)
        rgb, shade, hits = res[0], res[1], res[2]
        assert np.array_equal(rgb, ref["frame"]) and np.array_equal(shade["rgb8"], rgb), where(rgb, ref["frame"])
        assert np.array_equal(hits["prim"][:, :, 0], ref["tri"]), "hit primitives differ"
        dg.same_floats(shade["linear"], ref["lin"], allowed[:, :, None], "rtx_render_view's linear colour")
        rows = scene.render_view_rows(view, stats=stats)
        if stats:
            assert res[3]["primary_hits"] == ref["stats"]["primary_hits"] and res[3]["shadow_rays"] == ref["stats"]["shadow_rays"]
            rows, rst = rows
            assert rst["primary_hits"] == ref["stats"]["primary_hits"] and rst["shadow_rays"] == ref["stats"]["shadow_rays"]
        assert np.array_equal(rows, ref["frame"]), "rtx_render_view_rows differs at %s" % where(rows, ref["frame"])


def test_thicket_under_every_probe_split_mode(orc, samples_seeded, scenes):
    scene, ref = scenes("thicket")["scene"], dg.thicket_frame(orc, samples_seeded)
    predicted = len(scene.probe_long()[0])
    same_under_every_mode(scene, rows_of(scene), ref["frame"], {0: predicted, 1: 0, 2: frame_tiles(scene.width, scene.height)})


@pytest.mark.parametrize("nb_ray", [1, 2])
def test_soup_frames(rtx, orc, samples_seeded, scenes, nb_ray):
    m = scenes("soup2" if nb_ray == 2 else "soup")
    scene, ref = m["scene"], dg.soup_frame(orc, samples_seeded, nb_ray)
    img, st = gpu_forms.render_both(scene)
    assert np.array_equal(img, ref["frame"]), "rtx_render_rows differs from the oracle at (y, x) %s" % where(img, ref["frame"])
    assert st["primary_hits"] == ref["stats"]["primary_hits"] and st["shadow_rays"] == ref["stats"]["shadow_rays"], st
    view = scene.own_view()
    rgb, shade, hits, vst = scene.render_view(view, stats=True, want_shade=True, want_hits=True)
    assert np.array_equal(rgb, ref["frame"]) and np.array_equal(shade["rgb8"], rgb), where(rgb, ref["frame"])
    assert vst["primary_hits"] == ref["stats"]["primary_hits"] and vst["shadow_rays"] == ref["stats"]["shadow_rays"]
    if nb_ray == 1:
        assert np.array_equal(hits["prim"][:, :, 0], ref["tri"]), "hit primitives differ"
    assert np.array_equal(scene.render_view(view), ref["frame"])
    rows, rst = scene.render_view_rows(view, stats=True)
    assert np.array_equal(rows, ref["frame"]) and np.array_equal(scene.render_view_rows(view), rows)
    assert rst["primary_hits"] == ref["stats"]["primary_hits"] and rst["shadow_rays"] == ref["stats"]["shadow_rays"]


# ---------------------------------------------------------------------------------------------- ray queries
def ray_set(orc, samples, name, key):
    rs = dg.ray_sets(orc, samples, "soup" if name.startswith("soup") else "thicket")
    return rs["mixed"][:3] + (None,) if key == "mixed" else dg.as_trace(rs[key])


@pytest.mark.parametrize("key", ["exposed", "grazing", "mixed"])
@pytest.mark.parametrize("name", ["thicket", "soup", "always", "never"])
def test_trace_rays(orc, samples_seeded, scenes, name, key):
    """prim, t and p_hit bits, normals by the NaN rule; the three reference_tree settings agree: no ray here is hard"""
    m = scenes(name)
    o, d, exp, _ = ray_set(orc, samples_seeded, name, key)
    what = "%s %s" % (name, key)
    got = trace_every_way(m["scene"], o, d, exp, None, what)
    check_normals(got, exp, m["tables"], m["nan"], what)
    if key == "exposed":
        c3 = m["prims"]["form_at"][exp["prim"]] == 5
        assert c3.sum() >= dg.MIN_PER_CLASS and np.isfinite(got["normal"][c3]).all()
        assert np.array_equal(bits(got["normal"][c3]), bits(m["tables"]["normals"][exp["prim"][c3]])), "a C3 triangle's stored normal"
    for n in SIZES:
        for kw in OPTIONS:
            part = m["scene"].trace_rays(o[:n], d[:n], **kw)
            assert part.tobytes() == got[:n].tobytes(), "%s: the first %d rays alone, %s" % (what, n, kw)
        tail = m["scene"].trace_rays(o[-n:], d[-n:], keep_order=True)
        assert tail.tobytes() == got[-n:].tobytes(), "%s: the last %d rays alone" % (what, n)


@pytest.mark.parametrize("name", ["thicket", "soup"])
def test_device_resident_queries_with_guard_bytes(rtx, orc, samples_seeded, scenes, name):
    torch = pytest.importorskip("torch")
    assert torch.cuda.is_available(), "torch sees no GPU"
    m = scenes(name)
    o, d, exp, _ = ray_set(orc, samples_seeded, name, "exposed")
    po, pt, _, want = dg.occlusion_pairs(orc, samples_seeded, name)["pairs"]
    stream = torch.cuda.current_stream().cuda_stream
    for n in (65, len(o)):
        t_o, t_d = torch.from_numpy(o[:n].copy()).to("cuda:0"), torch.from_numpy(d[:n].copy()).to("cuda:0")
        t_po, t_pt = torch.from_numpy(po[:n].copy()).to("cuda:0"), torch.from_numpy(pt[:n].copy()).to("cuda:0")
        hits = torch.full((n * 32 + 64,), 0xAA, dtype=torch.uint8, device="cuda:0")
        occ = torch.full((n + 64,), 0xAA, dtype=torch.uint8, device="cuda:0")
        shade = torch.full((n * 16 + 64,), 0xAA, dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
        for kw in OPTIONS:
            m["scene"].trace_rays_device(0, n, t_o.data_ptr(), t_d.data_ptr(), hits.data_ptr(), stream, **kw)
            m["scene"].occluded_rays_device(0, n, t_po.data_ptr(), t_pt.data_ptr(), occ.data_ptr(), stream, **kw)
            m["scene"].shade_rays_device(0, n, t_o.data_ptr(), t_d.data_ptr(), shade.data_ptr(), None, stream, **kw)
            torch.cuda.synchronize()
            h, c, s = hits.cpu().numpy(), occ.cpu().numpy(), shade.cpu().numpy()
            assert (h[n * 32:] == 0xAA).all() and (c[n:] == 0xAA).all() and (s[n * 16:] == 0xAA).all(), "guard bytes"
            got = h[:n * 32].view(rtx.rtx.RAY_HIT_DTYPE)
            qs.check_hits(got, exp[:n], None, "%s device-resident %d %s" % (name, n, kw))
            check_normals(got, exp[:n], m["tables"], m["nan"], "%s device-resident %d" % (name, n))
            assert np.array_equal(c[:n], want[:n]), (name, n, kw)
            assert s[:n * 16].tobytes() == m["scene"].shade_rays(o[:n], d[:n], keep_order=True).tobytes(), (name, n, kw)


def mixed_pairs(orc, samples, name):
    """the mixed set as pairs (origin, origin + direction), answered by the oracle along fl(target - origin)"""
    def make():
        rs = dg.ray_sets(orc, samples, name)
        mo, md = rs["mixed"][0], rs["mixed"][1]
        return qs.pair_sets(orc, rs["osc"], mo, (mo + md).astype(F))["occlusion"]
    return qs._once("deg_mixed_pairs_" + name, make)


@pytest.mark.parametrize("name", ["thicket", "soup", "always", "never"])
def test_occluded_rays(orc, samples_seeded, scenes, name):
    m = scenes(name)
    pr = dg.occlusion_pairs(orc, samples_seeded, "soup" if name == "soup" else "thicket")
    o, t, _, want = pr["pairs"]
    assert want[:pr["n_exposed"]].all()
    occluded_every_way(m["scene"], o, t, want, name + " pairs")
    for n in SIZES:
        for kw in OPTIONS:
            assert np.array_equal(m["scene"].occluded_rays(o[:n], t[:n], **kw), want[:n]), (name, n, kw)
    mixed = mixed_pairs(orc, samples_seeded, "soup" if name == "soup" else "thicket")
    occluded_every_way(m["scene"], mixed[0], mixed[1], mixed[3], name + " mixed pairs")


@pytest.mark.parametrize("key", ["exposed", "mixed"])
@pytest.mark.parametrize("name", ["thicket", "soup", "always", "never"])
def test_shade_rays(orc, samples_seeded, scenes, name, key):
    m = scenes(name)
    s = dg.shade_batch(orc, samples_seeded, "soup" if name == "soup" else "thicket", key)
    o, d = s["origins"], s["directions"]
    traced = m["scene"].trace_rays(o, d, keep_order=True)
    qs.check_hits(traced, s["hit"], None, "%s %s" % (name, key))
    first = None
    for kw in OPTIONS:
        for stats in (False, True):
            res = m["scene"].shade_rays(o, d, want_hits=True, stats=stats, **kw)
            check_shade(res[0], res[1], s, traced, m["nan"], "%s %s %s" % (name, key, kw))
            first = res[0] if first is None else first
            assert res[0].tobytes() == first.tobytes(), (name, key, kw, stats)
            if stats:
                n_hits = int((s["hit"]["prim"] != NO_HIT).sum())
                count = s["samples"].sum() // max(n_hits, 1)
                assert res[2]["primary_hits"] == n_hits and res[2]["shadow_rays"] == count * n_hits, res[2]
    for n in SIZES:
        assert m["scene"].shade_rays(o[:n], d[:n], keep_order=True).tobytes() == first[:n].tobytes(), (name, key, n)


# ---------------------------------------------------------------------------------------------- 1 x 1 frames
def test_one_pixel_frames(rtx, orc, samples_half):
    """one pixel is one lane: rtx_render_rows (with and without statistics), rtx_render_view with hit records and
    rtx_render_view_rows of a scene created with each camera, against the oracle scene of that camera"""
    prims = dg.thicket(orc)
    nan = dg.nan_prims(prims)
    for f in dg.frames(orc, samples_half)["frames"]:
        what = "a 1 x 1 frame onto a %s triangle" % dg.FORMS[f["form"]]
        with dg.open_scene(rtx, samples_half, prims, f["view"]) as scene:
            img, st = gpu_forms.render_both(scene)
            assert img.shape == (1, 1, 3) and np.array_equal(img, f["ref"]), "%s: rtx_render_rows gives %s, the oracle %s" \
                % (what, img[0, 0].tolist(), f["ref"][0, 0].tolist())
            assert st["primary_rays"] == 1 and st["primary_hits"] == 1 and st["shadow_rays"] == f["stats"]["shadow_rays"], (what, st)
            view = scene.own_view()
            for stats in (True, False):
                res = scene.render_view(view, stats=stats, want_shade=True, want_hits=True)
                qs.check_hits(res[2].reshape(-1), f["exp"], None, what + ": rtx_render_view's hit record")
                assert np.array_equal(res[0], f["ref"]) and np.array_equal(res[1]["rgb8"], res[0]), what
                dg.same_floats(res[1]["linear"], f["lin"], nan[f["exp"]["prim"]][:, None, None], what + ": linear")
                rows = scene.render_view_rows(view, stats=stats)
                rows = rows[0] if stats else rows
                assert np.array_equal(rows, f["ref"]), what + ": rtx_render_view_rows gives %s" % rows[0, 0].tolist()


# ---------------------------------------------------------------------------------------------- poses: the words
def same_shade_words(got, want, nan, what):
    """shading records [n, 8]: the three normal words by the NaN rule, the other five word for word"""
    dg.same_floats(got.view(F)[:, 0:3], want.view(F)[:, 0:3], nan[:, None], what + ": normals")
    bad = np.argwhere(got[:, 3:] != want[:, 3:])
    assert not len(bad), "%s: shading words differ at %s" % (what, bad[:6].tolist())


def check_device(scene, given, nan, what, rebuilt, eye=dg.THICKET_VIEW[1]):
    """test_gpu_prims.check_device with the NaN rule for the normals: the pose the device holds against
    rtx_scene_pose_prims_records / _aimed and the plane records, read back by the debug readers"""
    aimed = scene.pose_prims_aimed(eye, rebuilt=rebuilt, **given)
    if rebuilt:
        keys, perm, t, s, n = scene.pose_prims_records(rebuilt=True, **given)
        dperm, dt, ds, dn, daimed = scene.debug_pose_rebuilt(eye=eye)
        same_words((dt, None, dn, daimed, dperm), (t, None, n, aimed, perm), what + ", rebuilt")
    else:
        t, s, n = scene.pose_prims_records(**given)
        dt, ds, dn = scene.debug_pose()
        planes, daimed = scene.debug_pose_pipeline(eye=eye)
        same_words((dt, None, dn, daimed), (t, None, n, aimed), what + ", refitted")
        v = scene.tris if given.get("v0v1v2") is None else given["v0v1v2"]
        assert np.array_equal(planes, scene.posed_pipeline_records(v)[0]), what + ": plane records"
    same_shade_words(ds, s, nan, what)


@pytest.mark.parametrize("name", dg.POSES)
def test_device_words_are_the_hosts_on_the_thicket(rtx, orc, scenes, name):
    torch = pytest.importorskip("torch")
    scene = scenes("thicket")["scene"]
    given = dg.given(orc, name)
    nan = dg.nan_prims(dg.pose(orc, name))
    kw, keep = on_device(torch, given)
    stream = torch.cuda.Stream(device="cuda:0")
    with torch.cuda.stream(stream):
        for rebuilt in (False, True):
            scene.pose_prims(rebuilt=rebuilt, **given)
            check_device(scene, given, nan, name + ", host variant", rebuilt)
            scene.pose_prims_device(0, rebuilt=rebuilt, stream=stream.cuda_stream, **kw)
            check_device(scene, given, nan, name + ", device variant", rebuilt)
            if name != "prims_all":                            # the plain calls state the same words
                (scene.pose_rebuilt if rebuilt else scene.pose)(given["v0v1v2"])
                check_device(scene, given, nan, name + ", plain call", rebuilt)
                (scene.pose_rebuilt_device if rebuilt else scene.pose_device)(0, kw["d_v0v1v2_ptr"], None, stream.cuda_stream)
                check_device(scene, given, nan, name + ", plain device call", rebuilt)
        stream.synchronize()


def test_device_words_are_the_hosts_on_the_size_scenes(rtx, samples_seeded):
    """posed onto one point, then back: runs of equal boxes and equal keys on either side of both refit thresholds"""
    torch = pytest.importorskip("torch")
    stream = torch.cuda.Stream(device="cuda:0")
    eye = dg.axis_view()["eye"]
    with torch.cuda.stream(stream):
        for name, sc in dg.size_scenes().items():
            with dg.open_sized(rtx, samples_seeded, sc) as scene:
                for pose, what in ((sc["pose"], "onto one point"), (sc["tris"], "back"), (sc["pose"], "onto one point again")):
                    given = dict(v0v1v2=pose, spheres=None, rgb=None, sphere_rgb=None)
                    flat = pose.reshape(-1, 3, 3)
                    nan = ~(np.linalg.norm(np.cross((flat[:, 1] - flat[:, 0]).astype(np.float64), (flat[:, 2] - flat[:, 0]).astype(np.float64)),
                                           axis=1) > 0)
                    kw, keep = on_device(torch, given)
                    for rebuilt in (False, True):
                        scene.pose_prims(rebuilt=rebuilt, **given)
                        check_device(scene, given, nan, "%s %s, host variant" % (name, what), rebuilt, eye)
                        scene.pose_prims_device(0, rebuilt=rebuilt, stream=stream.cuda_stream, **kw)
                        check_device(scene, given, nan, "%s %s, device variant" % (name, what), rebuilt, eye)
                    stream.synchronize()


# ---------------------------------------------------------------------------------------------- poses: frames and queries
def check_posed_frame(scene, view, p, nan, what, light=None):
    hit = p["tri"] != NO_HIT
    allowed = hit & nan[np.where(hit, p["tri"], 0)]
    rgb, shade, hits, st = scene.render_view(view, stats=True, want_shade=True, want_hits=True, posed=True)
    assert np.array_equal(rgb, p["frame"]), "%s: bytes differ from the oracle scene at (y, x) %s" % (what, where(rgb, p["frame"]))
    assert np.array_equal(shade["rgb8"], rgb) and np.array_equal(hits["prim"][:, :, 0], p["tri"]), what + ": hit primitives differ"
    dg.same_floats(shade["linear"], p["lin"], allowed[:, :, None], what + ": linear")
    assert st["primary_hits"] == p["stats"]["primary_hits"] and st["shadow_rays"] == p["stats"]["shadow_rays"], (what, st)
    rows, rst = scene.render_view_rows(view, stats=True, posed=True)
    assert np.array_equal(rows, p["frame"]), "%s: rows differ from the oracle scene at (y, x) %s" % (what, where(rows, p["frame"]))
    assert rst["primary_hits"] == p["stats"]["primary_hits"] and rst["shadow_rays"] == p["stats"]["shadow_rays"], (what, rst)
    assert np.array_equal(scene.render_view_rows(view, posed=True), rows)
    return rgb.tobytes(), hits["prim"].tobytes(), rows.tobytes()


@pytest.mark.parametrize("name", dg.POSES)
def test_posed_views_and_rows_are_the_oracle_scene_with_the_posed_primitives(rtx, orc, samples_seeded, scenes, name):
    scene = scenes("thicket")["scene"]
    p = dg.posed(orc, samples_seeded, name)
    nan = dg.nan_prims(p["prims"])
    view = scene.own_view()
    seen = []
    for rebuilt in (False, True):
        scene.pose_prims(rebuilt=rebuilt, **dg.given(orc, name))
        seen.append(check_posed_frame(scene, view, p, nan, "%s, %s" % (name, "rebuilt" if rebuilt else "refitted")))
    assert seen[0] == seen[1], name + ": refitted and rebuilt differ"
    base = dg.thicket_frame(orc, samples_seeded)["frame"]
    assert np.array_equal(scene.render_view_rows(view), base) and np.array_equal(scene.render_rows(), base), "the unposed scene changed"


def test_posed_queries_on_folds_own_exposed_set(rtx, orc, samples_seeded, scenes):
    scene = scenes("thicket")["scene"]
    rs = dg.ray_sets(orc, samples_seeded, "fold")
    tb, nan = dg.tables_of(orc, rs["prims"]), dg.nan_prims(rs["prims"])
    pr = dg.occlusion_pairs(orc, samples_seeded, "fold")["pairs"]
    sets = dict(exposed=dg.as_trace(rs["exposed"]), grazing=dg.as_trace(rs["grazing"]), mixed=rs["mixed"][:3] + (None,))
    shades = {key: dg.shade_batch(orc, samples_seeded, "fold", key) for key in ("exposed", "mixed")}
    for rebuilt in (False, True):
        scene.pose_prims(rebuilt=rebuilt, **dg.given(orc, "fold"))
        for key, (o, d, exp, _) in sets.items():
            for n in SIZES + (len(o),):
                for kw in OPTIONS:
                    got = scene.trace_rays(o[:n], d[:n], posed=True, **kw)
                    qs.check_hits(got, exp[:n], None, "fold %s %d %s" % (key, n, kw))
                    check_normals(got, exp[:n], tb, nan, "fold %s %d %s" % (key, n, kw))
        for n in SIZES + (len(pr[0]),):
            for kw in OPTIONS:
                got = scene.occluded_rays(pr[0][:n], pr[1][:n], posed=True, **kw)
                assert np.array_equal(got, pr[3][:n]), ("fold pairs", n, kw, np.nonzero(got != pr[3][:n])[0][:8])
        for key, s in shades.items():
            traced = scene.trace_rays(s["origins"], s["directions"], keep_order=True, posed=True)
            for kw in OPTIONS:
                got, hits = scene.shade_rays(s["origins"], s["directions"], want_hits=True, posed=True, **kw)
                check_shade(got, hits, s, traced, nan, "fold %s %s" % (key, kw))


def test_nothing_of_a_previous_pose_survives(rtx, orc, samples_seeded, scenes):
    """collapse, then unfold, then a plain pose, on one scene"""
    scene = scenes("thicket")["scene"]
    view = scene.own_view()
    for rebuilt in (False, True):
        for name in ("prims_all", "collapse", "unfold"):
            p = dg.posed(orc, samples_seeded, name)
            scene.pose_prims(rebuilt=rebuilt, **dg.given(orc, name))
            check_posed_frame(scene, view, p, dg.nan_prims(p["prims"]), "%s in sequence" % name)
        p = dg.posed(orc, samples_seeded, "fold")
        (scene.pose_rebuilt if rebuilt else scene.pose)(p["prims"]["tris"])                    # a plain pose: vertices alone
        check_posed_frame(scene, view, p, dg.nan_prims(p["prims"]), "a plain fold after unfold")
        check_device(scene, dg.given(orc, "fold"), dg.nan_prims(p["prims"]), "a plain fold after unfold", rebuilt)


# ---------------------------------------------------------------------------------------------- lights
@pytest.mark.parametrize("light_name", list(dg.LIGHTS))
def test_degenerate_lights(rtx, orc, samples_seeded, scenes, light_name):
    m = scenes("thicket")
    scene = m["scene"]
    light = rtx.Scene.make_light(dg.LIGHTS[light_name], dg.NB_LIGHT)
    view = scene.own_view()
    assert np.array_equal(bits(scene.debug_light_points(light)), bits(scene.light_points_for(light))), light_name
    check_walk(scene, light, light_name)
    frame, ost = dg.lit(orc, samples_seeded, "thicket", light_name)
    rgb, st = scene.render_view(view, stats=True, light=light)
    assert np.array_equal(rgb, frame), "%s: the lit view differs from the oracle scene at %s" % (light_name, where(rgb, frame))
    assert st["shadow_rays"] == ost["shadow_rays"]
    rows = scene.render_view_rows(view, light=light)
    assert np.array_equal(rows, frame), "%s: the lit rows differ from the oracle scene at %s" % (light_name, where(rows, frame))
    s = dg.shade_batch(orc, samples_seeded, "thicket", "exposed", light=light_name)
    traced = scene.trace_rays(s["origins"], s["directions"], keep_order=True)
    for kw in OPTIONS:
        got, hits = scene.shade_rays(s["origins"], s["directions"], want_hits=True, light=light, **kw)
        check_shade(got, hits, s, traced, m["nan"], "%s light, exposed %s" % (light_name, kw))
    # under fold
    p = dg.posed(orc, samples_seeded, "fold")
    frame, ost = dg.lit(orc, samples_seeded, "fold", light_name)
    s = dg.shade_batch(orc, samples_seeded, "fold", "exposed", light=light_name)
    nan = dg.nan_prims(p["prims"])
    for rebuilt in (False, True):
        scene.pose_prims(rebuilt=rebuilt, **dg.given(orc, "fold"))
        rgb, st = scene.render_view(view, stats=True, light=light, posed=True)
        assert np.array_equal(rgb, frame) and st["shadow_rays"] == ost["shadow_rays"], "%s, fold: the lit view at %s" % (light_name, where(rgb, frame))
        rows = scene.render_view_rows(view, light=light, posed=True)
        assert np.array_equal(rows, frame), "%s, fold: the lit rows at %s" % (light_name, where(rows, frame))
        traced = scene.trace_rays(s["origins"], s["directions"], keep_order=True, posed=True)
        got, hits = scene.shade_rays(s["origins"], s["directions"], want_hits=True, light=light, posed=True, keep_order=True)
        check_shade(got, hits, s, traced, nan, "%s light, fold, exposed" % light_name)
    assert np.array_equal(scene.render_view_rows(view), dg.thicket_frame(orc, samples_seeded)["frame"]), "the scene's own light afterwards"
