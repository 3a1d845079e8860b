"""GPU parity of a scene whose sample table is replaced (rtx_scene_resample, rtx_scene_reseed; the sample-table kernel and
each device's catch-up): the device's table word for word against the host statement, and every render, view, shade, lit and
posed call after a replacement against an ORACLE SCENE CREATED WITH THE NEW TABLE (tests/resample_sets.py, whose conditions
tests/test_resample_sets.py asserts without a GPU: every table changes its frame, B by the jitter alone and C by the light
points alone).  Every comparison is for equal bits or bytes."""
import importlib

import numpy as np
import pytest

import moves_sets as mv
import prims_sets as pm
import query_sets as qs
import resample_sets as rs
import sequence_sets as sq
import skin_sets as sk
import view_sets as vs
from query_sets import F, bits

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def rtx():
    mod = importlib.import_module("ray-tracer-rust_amd")
    assert mod.device_count() >= 1, "no HIP device: the product path has no CPU fallback"
    return mod


def lib_view(rtx, v=pm.YARD_VIEW):
    (w, h) = v[0]
    return rtx.Scene.view(w, h, **vs.camera(v))


def where(got, want):
    return np.argwhere((got != want).any(axis=2))[:8].tolist()


def same_frame(got, want, what):
    assert np.array_equal(got, want), "%s: bytes differ from the oracle scene at (y, x) %s" % (what, where(got, want))


def tiles_frame(torch, scene):
    """the scene's own frame through rtx_render_tiles_device: one share of 8-row tiles, into a guarded device buffer"""
    n = scene.tiles_bytes(0, 1, 8)
    buf = torch.full((n + 16,), 0xAA, dtype=torch.uint8, device="cuda:0")
    scene.render_tiles_device(0, 0, 1, 8, buf.data_ptr(), n, torch.cuda.current_stream().cuda_stream, None)
    torch.cuda.synchronize()
    out = buf.cpu().numpy()
    assert (out[n:] == 0xAA).all()
    return out[:n].reshape(scene.height, scene.width, 3)


def check_every_entry_point(torch, rtx, scene, r, what):
    """the yard's scene against the oracle scene's render `r` (resample_sets.yard_render)"""
    view = lib_view(rtx)
    rows, st = scene.render_rows(stats=True)
    same_frame(rows, r["frame"], what + ", rtx_render_rows")
    assert st["primary_hits"] == r["stats"]["primary_hits"] and st["shadow_rays"] == r["stats"]["shadow_rays"], (what, st)
    same_frame(scene.render_frame(devices=(0, 0, 0), tile_rows=8), r["frame"], what + ", rtx_render_frame")
    same_frame(tiles_frame(torch, scene), r["frame"], what + ", rtx_render_tiles_device")
    rgb, shade, hits, vst = scene.render_view(view, stats=True, want_shade=True, want_hits=True)
    same_frame(rgb, r["frame"], what + ", rtx_render_view")
    assert np.array_equal(bits(shade["linear"]), bits(r["lin"])), what + ": linear words differ from the oracle scene's"
    assert np.array_equal(shade["rgb8"], rgb) and np.array_equal(hits["prim"][:, :, 0], r["tri"]), what + ": records"
    assert vst["primary_hits"] == r["stats"]["primary_hits"]
    vrows, rst = scene.render_view_rows(view, stats=True)
    same_frame(vrows, r["frame"], what + ", rtx_render_view_rows")
    assert rst["primary_hits"] == r["stats"]["primary_hits"] and rst["shadow_rays"] == r["stats"]["shadow_rays"]
    o, d = r["rays"]
    h, w = r["frame"].shape[:2]
    for kw in (dict(keep_order=True), dict(force_regroup=True)):
        s = scene.shade_rays(o, d, **kw)
        same_frame(s["rgb8"].reshape(h, w, 3), r["frame"], what + ", rtx_shade_rays %s" % kw)
        assert np.array_equal(bits(s["linear"].reshape(h, w, 3)), bits(r["lin"])), (what, kw)


# ---------------------------------------------------------------------------------------------- 1: the table itself
@pytest.mark.parametrize("seed", rs.SEEDS)
def test_the_devices_table_is_the_statement(rtx, orc, seed):
    with rs.open_yard(rtx, rs.tables(orc)["A"]) as scene:
        assert np.array_equal(bits(scene.debug_samples()), bits(rs.tables(orc)["A"]))           # as created
        for n in rs.KERNEL_PAIRS:
            scene.reseed(seed, n)
            want = rtx.gen_samples(seed, n)
            got = scene.debug_samples()
            assert got.shape == (n, 2) and np.array_equal(bits(got), bits(want)), (seed, n, np.argwhere(bits(got) != bits(want))[:6].tolist())
            assert np.array_equal(bits(scene.debug_samples(n - 1, 1)), bits(want[-1:])), (seed, n)
            if n > 3:
                assert np.array_equal(bits(scene.debug_samples(n - 3, 3)), bits(want[-3:])), (seed, n)
            assert np.array_equal(bits(got), bits(scene.samples_at()))
            out = np.zeros((2, 2), F)
            rc = rtx.rtx._lib.rtx_debug_samples(scene.handle, 0, n - 1, 2, out.ctypes.data_as(rtx.rtx.f32p))      # straddles the end
            assert rc == rtx.ERR_BAD_ARG and not out.any()


def test_a_whole_table_of_two_million_pairs_and_a_callers(rtx, orc):
    t = rs.tables(orc)
    with rs.open_yard(rtx, t["A"]) as scene:
        scene.reseed(rs.SEEDS[3], rs.WHOLE_PAIRS)
        want = rtx.gen_samples(rs.SEEDS[3], rs.WHOLE_PAIRS)
        got = scene.debug_samples()
        assert np.array_equal(bits(got), bits(want)), np.argwhere(bits(got) != bits(want))[:6].tolist()
        assert np.array_equal(bits(scene.debug_samples(rs.WHOLE_PAIRS - 1, 1)), bits(want[-1:]))
        other = rtx.gen_samples(99, rs.WHOLE_PAIRS)
        scene.resample(other)                                      # the same buffer, now by a copy
        assert np.array_equal(bits(scene.debug_samples()), bits(other))
        for name in ("D1", "D7", "Dbig", "inf"):                     # a caller's table, entries that are not finite included
            scene.resample(t[name])
            assert np.array_equal(bits(scene.debug_samples()), bits(t[name])), name
        scene.upload()                                               # nothing to catch up with: the table stands
        assert np.array_equal(bits(scene.debug_samples(3, 1)), bits(t["inf"][3:4]))


# ---------------------------------------------------------------------------------------------- 2: entry points
@pytest.mark.parametrize("name", rs.RENDERED)
def test_every_entry_point_after_a_resample_is_the_oracle_scene_with_the_table(rtx, orc, samples_seeded, name):
    torch = pytest.importorskip("torch")
    t = rs.tables(orc)
    with rs.open_yard(rtx, t["A"]) as scene:
        own = rs.yard_render(orc, rtx, samples_seeded, "A")
        same_frame(scene.render_rows(), own["frame"], "as created")                 # the device holds A, and has launched
        rs.apply(scene, orc, name)
        r = rs.yard_render(orc, rtx, samples_seeded, name)
        assert (r["frame"] != own["frame"]).any()
        check_every_entry_point(torch, rtx, scene, r, "resampled to " + name)
        assert np.array_equal(bits(scene.debug_samples()), bits(t[name]))
    with rs.open_yard(rtx, t["A"]) as fresh:                                         # resampled before the first upload
        rs.apply(fresh, orc, name)
        same_frame(fresh.render_view_rows(lib_view(rtx)), r["frame"], "resampled to %s before the upload" % name)
        same_frame(fresh.render_rows(), r["frame"], "resampled to %s before the upload, rows" % name)


def test_ray_queries_return_what_they_returned(rtx, orc, samples_seeded):
    (ro, rd, exp), (to, tt, texp, occ) = rs.yard_queries(orc, rtx, samples_seeded)
    with rs.open_yard(rtx, rs.tables(orc)["A"]) as scene:
        before = scene.trace_rays(ro, rd).tobytes(), scene.occluded_rays(to, tt).tobytes()
        qs.check_hits(scene.trace_rays(ro, rd), exp, None, "as created")
        for name in ("C", "seed_max", "D1"):
            rs.apply(scene, orc, name)
            assert (scene.trace_rays(ro, rd).tobytes(), scene.occluded_rays(to, tt).tobytes()) == before, name
            assert np.array_equal(scene.occluded_rays(to, tt, keep_order=True), occ), name


# ---------------------------------------------------------------------------------------------- 3: lit calls
@pytest.mark.parametrize("name", ["B", "C", "D7", "seed_1"])
def test_lit_calls_read_the_new_table(rtx, orc, samples_seeded, name):
    view = lib_view(rtx)
    light = rtx.Scene.make_light(*rs.YARD_LIGHT)
    with rs.open_yard(rtx, rs.tables(orc)["A"]) as scene:
        lit_own = rs.yard_render(orc, rtx, samples_seeded, "A", light=rs.YARD_LIGHT)
        same_frame(scene.render_view_rows(view, light=light), lit_own["frame"], "lit rows as created")
        rs.apply(scene, orc, name)
        lit, r = rs.yard_render(orc, rtx, samples_seeded, name, light=rs.YARD_LIGHT), rs.yard_render(orc, rtx, samples_seeded, name)
        rgb, shade = scene.render_view(view, want_shade=True, light=light)
        same_frame(rgb, lit["frame"], "lit view after " + name)
        assert np.array_equal(bits(shade["linear"]), bits(lit["lin"]))
        same_frame(scene.render_view_rows(view, light=light), lit["frame"], "lit rows after " + name)
        o, d = r["rays"]
        s = scene.shade_rays(o, d, light=light)
        same_frame(s["rgb8"].reshape(rgb.shape), lit["frame"], "lit shade after " + name)
        # the device's points and walk of that light against the host's, which read the same table
        assert np.array_equal(bits(scene.debug_light_points(light)), bits(scene.light_points_for(light)))
        # the scene's own light given as a light: the unlit call
        mine = scene.light()
        same_frame(scene.render_view(view, light=mine), r["frame"], "own light, view")
        same_frame(scene.render_view_rows(view, light=mine), r["frame"], "own light, rows")
        assert scene.shade_rays(o, d, light=mine).tobytes() == scene.shade_rays(o, d).tobytes()


@pytest.mark.parametrize("name", rs.BUNNY_TABLES)
def test_the_bunny_under_its_own_and_the_fixture_light(rtx, orc, name):
    t = rs.tables(orc)
    v = lib_view(rtx, rs.BUNNY_VIEW)
    light = rtx.Scene.make_light(*rs.BUNNY_LIGHT)
    with rs.open_bunny(rtx, t["A"]) as scene:
        same_frame(scene.render_rows(), rs.bunny_render(orc, "A")["frame"], "bunny as created")
        same_frame(scene.render_view_rows(v, light=light), rs.bunny_render(orc, "A", lit=True)["frame"], "bunny lit as created")
        rs.apply(scene, orc, name)
        r, lit = rs.bunny_render(orc, name), rs.bunny_render(orc, name, lit=True)
        rows, st = scene.render_rows(stats=True)
        same_frame(rows, r["frame"], "bunny rows after " + name)
        assert st["primary_hits"] == r["stats"]["primary_hits"]
        same_frame(scene.render_frame(devices=(0, 0, 0), tile_rows=8), r["frame"], "bunny frame after " + name)
        same_frame(scene.render_view(v), r["frame"], "bunny view after " + name)
        same_frame(scene.render_view_rows(v), r["frame"], "bunny view rows after " + name)
        same_frame(scene.render_view(v, light=light), lit["frame"], "bunny lit view after " + name)
        same_frame(scene.render_view_rows(v, light=light), lit["frame"], "bunny lit rows after " + name)


# ---------------------------------------------------------------------------------------------- 4: standing state
@pytest.mark.parametrize("pose", rs.POSES)
@pytest.mark.parametrize("rebuilt", [False, True])
def test_a_pose_stands_through_a_resample(rtx, orc, samples_seeded, pose, rebuilt):
    view = lib_view(rtx)
    kind, pname = pose
    t = rs.tables(orc)
    with rs.open_yard(rtx, t["A"]) as scene:
        if kind == "prims":
            scene.pose_prims(rebuilt=rebuilt, **pm.given(rtx, pname))
        elif kind == "moved":
            scene.pose_moved(rebuilt=rebuilt, **mv.moves(rtx, pname))
        else:
            scene.skin(**sk.skin(rtx, pname))
            scene.pose_skinned(rebuilt=rebuilt, **sk.moves(rtx, pname))
        words = lambda: [a for a in (scene.debug_pose_rebuilt() if rebuilt else scene.debug_pose()) if a is not None]
        before = [a.copy() for a in words()]
        same_frame(scene.render_view_rows(view, posed=True), rs.yard_render(orc, rtx, samples_seeded, "A", pose=pose)["frame"], "posed as created")
        for name in ("B", "seed_1", "C"):                                        # no pose call in between
            rs.apply(scene, orc, name)
            p = rs.yard_render(orc, rtx, samples_seeded, name, pose=pose)
            what = "%s %s, %s, after %s" % (kind, pname, "rebuilt" if rebuilt else "refitted", name)
            same_frame(scene.render_view_rows(view, posed=True), p["frame"], what + ", posed rows")
            rgb, shade = scene.render_view(view, want_shade=True, posed=True)
            same_frame(rgb, p["frame"], what + ", posed view")
            assert np.array_equal(bits(shade["linear"]), bits(p["lin"])), what
            assert all(np.array_equal(a, b) for a, b in zip(before, words())), what + ": the pose's words changed"
            same_frame(scene.render_view_rows(view), rs.yard_render(orc, rtx, samples_seeded, name)["frame"], what + ", unposed rows")


def test_aimed_streams_of_one_eye_around_a_resample(rtx, orc, samples_seeded):
    """posed and unposed view rows of one eye before and after: the aimed streams are kept (the device's aimed words are the
    same) and the bytes are the new table's"""
    view = lib_view(rtx)
    eye = pm.YARD_VIEW[1]
    pose = rs.POSES[0]
    with rs.open_yard(rtx, rs.tables(orc)["A"]) as scene:
        scene.pose_prims(**pm.given(rtx, pose[1]))
        for name in ("A", "C", "seed_0"):
            if name != "A":
                rs.apply(scene, orc, name)
            for k in range(2):
                same_frame(scene.render_view_rows(view), rs.yard_render(orc, rtx, samples_seeded, name)["frame"], "unposed, %s, %d" % (name, k))
                same_frame(scene.render_view_rows(view, posed=True), rs.yard_render(orc, rtx, samples_seeded, name, pose=pose)["frame"],
                           "posed, %s, %d" % (name, k))
            aimed = scene.debug_aimed_nodes(eye), scene.debug_pose_pipeline(eye=eye)[1]
            if name == "A":
                first = [a.copy() for a in aimed]
            assert all(np.array_equal(a, b) for a, b in zip(first, aimed)), name


# ---------------------------------------------------------------------------------------------- 5: hard rays, probe split
def test_a_tile_of_hard_rays_goes_through_the_reference_re_render(rtx, orc, samples_seeded):
    """sequence_sets' P — an axis camera and the all-zero table: the centre row's -0.0 direction components — created with
    ANOTHER table and resampled to the zero one: its reference frame, with tiles re-rendered; three rays per pixel"""
    ref = sq.reference("P", orc, samples_seeded, rtx)
    d = ref["desc"]
    tris, rgb, zeros = d["args"]
    assert not zeros.any() and sq.tiles_holding_a_hard_ray(ref, 0, d["H"]) > 0
    with sq.make_scene(rtx, dict(d, args=(tris, rgb, rtx.gen_samples(5, 4096)))) as scene:
        first, st = scene.render_rows(stats=True)
        assert (first != ref["frame"]).any()
        scene.resample(zeros)
        rows, st = scene.render_rows(stats=True)
        same_frame(rows, ref["frame"], "P resampled to the zero table")
        assert st["redo_tiles"] > 0 and st["primary_hits"] == int(ref["hits"].sum())
        same_frame(scene.render_view_rows(scene.own_view()), ref["frame"], "P resampled, view rows")
        same_frame(scene.render_frame(devices=(0, 0, 0), tile_rows=8), ref["frame"], "P resampled, frame")


def test_probe_split_modes_after_a_resample(rtx, orc):
    """the long list is kept as created: an ordering hint, so the prediction, no long tile and every tile long give equal
    bytes — the oracle scene's — after a resample"""
    t = rs.tables(orc)
    with rs.open_bunny(rtx, t["A"]) as scene:
        long_before = scene.probe_long()
        scene.render_rows()
        for name in rs.BUNNY_TABLES[:2]:
            rs.apply(scene, orc, name)
            want = rs.bunny_render(orc, name)["frame"]
            for mode in (0, 1, 2, 0):
                scene.debug_probe_split(mode)
                same_frame(scene.render_rows(), want, "bunny after %s, probe split mode %d" % (name, mode))
        assert all(np.array_equal(a, b) for a, b in zip(long_before, scene.probe_long()))


# ---------------------------------------------------------------------------------------------- 6: sequences
def test_sequences_of_tables(rtx, orc, samples_seeded):
    view = lib_view(rtx)
    t = rs.tables(orc)
    frame = lambda n: rs.yard_render(orc, rtx, samples_seeded, n)["frame"]
    with rs.open_yard(rtx, t["A"]) as scene, rs.open_yard(rtx, t["A"]) as other:
        created = scene.render_rows().tobytes(), scene.render_view(view).tobytes(), scene.render_view_rows(view).tobytes()
        # A -> B -> A restores the created scene's bytes
        scene.resample(t["B"])
        same_frame(scene.render_rows(), frame("B"), "B")
        scene.resample(t["A"])
        assert (scene.render_rows().tobytes(), scene.render_view(view).tobytes(), scene.render_view_rows(view).tobytes()) == created
        # resample then reseed, reseed then resample; a table that shrinks, then grows (the buffer grows once)
        for name in ("C", "seed_1", "D7", "seed_more", "D1", "Dbig", "seed_0", "half", "D1", "seed_max"):
            rs.apply(scene, orc, name)
            same_frame(scene.render_view_rows(view), frame(name), name + ", view rows")
            same_frame(scene.render_rows(), frame(name), name + ", rows")
            assert np.array_equal(bits(scene.debug_samples()), bits(t[name])), name
            # two live scenes, one of them resampled
            assert other.render_rows().tobytes() == created[0], name
        # two replacements with no call between them: the device catches up with the last
        scene.resample(t["B"])
        scene.reseed(rs.SEED_OF["seed_1"], rs.SEEDED_PAIRS)
        same_frame(scene.render_rows(), frame("seed_1"), "two replacements, one catch-up")
        # a refused call between two frames changes nothing
        L = rtx.rtx._lib
        assert L.rtx_scene_resample(scene.handle, None, 7) == rtx.ERR_BAD_ARG and L.rtx_scene_reseed(scene.handle, 1, 0) == rtx.ERR_BAD_ARG
        assert L.rtx_scene_resample(scene.handle, np.ascontiguousarray(t["B"]).ctypes.data_as(rtx.rtx.f32p), 0) == rtx.ERR_BAD_ARG
        same_frame(scene.render_rows(), frame("seed_1"), "after refused calls")
        assert np.array_equal(bits(scene.debug_samples()), bits(t["seed_1"]))
        other.resample(t["C"])
        same_frame(other.render_rows(), frame("C"), "the other scene")
        same_frame(scene.render_rows(), frame("seed_1"), "beside the other scene")


def test_device_resident_launches_around_a_resample(rtx, orc, samples_seeded):
    """launches on a caller's stream, a resample, launches again, nothing waited for by the caller in between: the catch-up
    waits for the device, so the first group's output is that of its own table"""
    torch = pytest.importorskip("torch")
    assert torch.cuda.is_available(), "torch sees no GPU"
    view = lib_view(rtx)
    n = view.ny * view.width * 3
    t = rs.tables(orc)
    frame = lambda name: rs.yard_render(orc, rtx, samples_seeded, name)["frame"]
    stream = torch.cuda.Stream(device="cuda:0")
    with rs.open_yard(rtx, t["A"]) as scene, torch.cuda.stream(stream):
        bufs = [torch.full((n + 16,), 0xAA, dtype=torch.uint8, device="cuda:0") for _ in range(6)]
        stream.synchronize()
        scene.render_view_rows_device(0, view, bufs[0].data_ptr(), bufs[0].numel(), stream.cuda_stream)
        scene.render_view_device(0, view, bufs[1].data_ptr(), None, None, stream.cuda_stream)
        scene.reseed(rs.SEED_OF["seed_0"], rs.SEEDED_PAIRS)
        scene.render_view_rows_device(0, view, bufs[2].data_ptr(), bufs[2].numel(), stream.cuda_stream)
        scene.render_view_device(0, view, bufs[3].data_ptr(), None, None, stream.cuda_stream)
        scene.resample(t["D7"])
        scene.render_view_rows_device(0, view, bufs[4].data_ptr(), bufs[4].numel(), stream.cuda_stream)
        scene.render_tiles_device(0, 0, 1, 8, bufs[5].data_ptr(), n, stream.cuda_stream, None)
        stream.synchronize()
        for name, b in zip(("A", "A", "seed_0", "seed_0", "D7", "D7"), bufs):
            out = b.cpu().numpy()
            assert out[:n].tobytes() == frame(name).tobytes() and (out[n:] == 0xAA).all(), name


# ---------------------------------------------------------------------------------------------- 7: an animation
def test_four_frames_of_reseed_and_posed_rows(rtx, orc, samples_seeded):
    """what the feature is for: per frame a new seeded table and a new skinned pose, through the posed pipeline"""
    view = lib_view(rtx)
    y = pm.yard(rtx)
    with rs.open_yard(rtx, rs.tables(orc)["A"]) as scene:
        scene.skin(**sk.skin(rtx, "bend"))
        moves = sk.moves(rtx, "bend")
        for k in range(4):
            m = moves["moves"].copy()
            m[:, 3] += F(1.5 * k)                                   # every move slides along x, frame by frame
            seed, pairs = 1000 + k, 4096 + 2 * k + 1
            scene.reseed(seed, pairs)
            scene.pose_skinned(m, rebuilt=bool(k & 1))
            v, sph = scene.skinned_prims(m)
            prims = dict(tris=v, rgb=y["rgb"], spheres=sph, sphere_rgb=y["sphere_rgb"])
            osc = rs.yard_oracle(orc, prims, orc.gen_samples(seed, pairs))
            want, _ = osc.render_rows(mode=orc.MODE_BVH)
            osc.close()
            same_frame(scene.render_view_rows(view, posed=True), want, "frame %d" % k)
            same_frame(scene.render_view(view, posed=True), want, "frame %d, view" % k)
