"""Model-based parity for sequences that pose, skin, relight and resample a live scene: one test per scene of
sequence_model.FAMILY.  Each runs its seeded operation log against rtx.Scene and checks EVERY observation against the CPU
oracle's answer on a fresh oracle scene created with the state a plain Python model says the library must be in
(tests/sequence_model.py; tests/test_sequence_model.py asserts, without a GPU, that the logs are worth running).

    frames          bytes equal to the oracle's render_rows(mode=MODE_BVH), primary_hits equal
    rays, shading   query_sets.oracle_hits / check_hits / check_normals, expected_occlusion and shade_sets.shade_set's
                    composition as they are: no tolerance of this file's own
    state changes   after a moved or skinned pose debug_moved_prims against the model's arrays and debug_pose /
                    debug_pose_rebuilt against pose_prims_records, word for word (always after a host variant; after a device
                    variant where the log drew it, so that device poses also run with nothing read between them and the next
                    call); after a table change debug_samples against samples_at and the model's table (where drawn)
    unposed calls   always the oracle scene of the created primitives under the current table

Device variants take torch tensors on one non-default stream of device 0, all made before the first call; nothing is
synchronised between calls until a device-resident observation's output is read.  With two devices the host variants draw
theirs from {0, 1}.  A failure's message carries the seed, the step and the whole log up to it: RTX_SEQUENCE_SEED and
RTX_SEQUENCE_STEPS replay it."""
import ctypes as C
import importlib
import time

import numpy as np
import pytest

import query_sets as qs
import sequence_model as sm
from query_sets import bits

pytestmark = pytest.mark.gpu
GUARD = 16


@pytest.fixture(scope="module")
def rtx():
    mod = importlib.import_module("ray-tracer-rust_amd")
    assert mod.device_count() >= 1, "no HIP device: the product path has no CPU fallback"
    return mod


def lib_view(rtx, v, rect=None):
    (w, h), eye, look_at, distance = v
    return rtx.Scene.view(w, h, eye, look_at, sm.UP, distance, rect=rect)


class Runner:
    def __init__(self, rtx, torch, scene, sc, draw, table):
        self.rtx, self.torch, self.scene, self.sc, self.draw = rtx, torch, scene, sc, draw
        self.model = sm.Model(sc, table, draw.n_devices)
        self.stream = torch.cuda.Stream(device="cuda:0")
        assert self.stream.cuda_stream != torch.cuda.default_stream().cuda_stream
        self.keep = {}                                          # step -> the tensors of a device variant, alive to the end
        with torch.cuda.stream(self.stream):
            for op in draw.log:
                if op.get("variant") == "device" or (op["op"] == "observe" and op["kind"].endswith("_device") and not op.get("refused")):
                    self.keep[op["step"]] = self.tensors(op)
        torch.cuda.synchronize()

    # -- the arrays of a device variant
    def on_device(self, a):
        a = np.ascontiguousarray(a)
        return self.torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).to("cuda:0")

    def tensors(self, op):
        t = {}
        if op["op"] == "observe":
            nb = self.sc["kw"]["nb_ray"]
            if op["kind"] == "shade_rays_device":
                t["origins"], t["second"] = self.on_device(op["origins"]), self.on_device(op["second"])
                n = len(op["origins"]) // nb * 16
            elif op["kind"] == "render_view_device":
                n = op["rect"][2] * op["rect"][3] * 3
                if op["want_shade"]:
                    t["shade"] = self.torch.full((op["rect"][2] * op["rect"][3] * 16 + GUARD,), 0xAA, dtype=self.torch.uint8, device="cuda:0")
            else:
                n = op["window"][1] * self.draw.views[op["view"]][0][0] * 3
            t["out"] = self.torch.full((n + GUARD,), 0xAA, dtype=self.torch.uint8, device="cuda:0")
            return t
        for k in ("tris", "spheres", "rgb", "sphere_rgb", "moves", "group", "radius_scale"):
            if op.get(k) is not None and np.size(op[k]):
                t[k] = self.on_device(op[k])
        return t

    # -- state changes
    def pose(self, op):
        s, dev, kind, reb = self.scene, op["dev"], op["op"], op["rebuilt"]
        if op["variant"] == "host":
            if kind == "pose":
                s.pose(op["tris"], device=dev)
            elif kind == "pose_rebuilt":
                s.pose_rebuilt(op["tris"], device=dev)
            elif kind == "pose_prims":
                s.pose_prims(op["tris"], op["spheres"], op["rgb"], op["sphere_rgb"], device=dev, rebuilt=reb)
            elif kind == "pose_moved":
                s.pose_moved(op["moves"], op["group"], op["radius_scale"], op["rgb"], op["sphere_rgb"], device=dev, rebuilt=reb)
            else:
                s.pose_skinned(op["moves"], op["radius_scale"], op["rgb"], op["sphere_rgb"], device=dev, rebuilt=reb)
            return
        t = self.keep[op["step"]]
        p = lambda k: t[k].data_ptr() if k in t else None
        st = self.stream.cuda_stream
        if kind == "pose":
            s.pose_device(0, p("tris"), None, st)
        elif kind == "pose_rebuilt":
            s.pose_rebuilt_device(0, p("tris"), None, st)
        elif kind == "pose_prims":
            s.pose_prims_device(0, p("tris"), p("spheres"), p("rgb"), p("sphere_rgb"), None, reb, st)
        elif kind == "pose_moved":
            s.pose_moved_device(0, len(op["moves"]), p("moves"), p("group"), p("radius_scale"), p("rgb"), p("sphere_rgb"), None, reb, st)
        else:
            s.pose_skinned_device(0, len(op["moves"]), p("moves"), p("radius_scale"), p("rgb"), p("sphere_rgb"), None, reb, st)

    def read_pose_back(self, op, what):
        s, dev, p = self.scene, op["dev"], self.model.pose[op["dev"]]
        if p["moved"]:
            for g, w, part in zip(s.debug_moved_prims(device=dev), (p["tris"], p["spheres"]), ("vertex", "sphere")):
                bad = np.argwhere(bits(g) != bits(w))
                assert not len(bad), "%s: %s words differ from the model's at %s" % (what, part, bad[:6].tolist())
        given = dict(v0v1v2=p["tris"], spheres=p["spheres"] if len(p["spheres"]) else None, rgb=p["rgb"] if len(p["rgb"]) else None,
                     sphere_rgb=p["sphere_rgb"] if len(p["sphere_rgb"]) else None)
        if p["rebuilt"]:
            _, perm, t, sh, n = s.pose_prims_records(rebuilt=True, **given)
            dperm, dt, ds, dn, _ = s.debug_pose_rebuilt(device=dev)
            assert np.array_equal(dperm, perm), what + ": permutation"
            got, want = (dt, ds, dn), (t, sh, n)
        else:
            got, want = s.debug_pose(device=dev), s.pose_prims_records(**given)
        for g, w, part in zip(got, want, ("primitive", "shading", "node")):
            bad = np.argwhere(g != w)
            assert not len(bad), "%s: %s words differ from pose_prims_records' at %s" % (what, part, bad[:6].tolist())

    def read_table_back(self, what):
        want = self.model.table_array()
        assert np.array_equal(bits(self.scene.samples_at()), bits(want)), what + ": samples_at differs from the model's table"
        for dev in range(self.draw.n_devices):
            got = self.scene.debug_samples(device=dev)
            bad = np.argwhere(bits(got) != bits(want))
            assert not len(bad), "%s: device %d's table differs at %s" % (what, dev, bad[:6].tolist())

    def refused(self, op, what):
        s, rtx = self.scene, self.rtx
        if op["refused"] == "skinned_with_group":               # (the binding's pose_skinned has no group to give)
            mvs, keep = s._moves_struct(op["moves"], op["group"], op["radius_scale"])
            code = rtx.rtx._lib.rtx_scene_pose_skinned(s.handle, op["dev"], C.byref(mvs), 1 if op["rebuilt"] else 0, rtx.REFTREE_NEVER, None)
            assert code == op["code"], "%s: %d" % (what, code)
            return
        with pytest.raises(rtx.RtxError) as e:
            if op["op"] == "observe":
                self.observe(op, None, what)
            elif op["op"] == "resample":
                s.resample(op["table"])
            else:
                self.pose(op)
        assert e.value.code == op["code"], "%s: %s" % (what, e.value)

    # -- observations
    def observe(self, ob, exp, what):
        s, rtx, k, dev = self.scene, self.rtx, ob["kind"], ob["dev"]
        v = self.draw.views[ob["view"]]
        (w, h) = v[0]
        light = None if ob.get("light") is None else rtx.Scene.make_light(*ob["light"])
        more = dict(light=light, posed=ob["posed"])
        order = dict(keep_order=ob.get("order") == "keep_order", force_regroup=ob.get("order") == "force_regroup")
        skip = exp is not None and exp["skip"]
        st = None

        def same_frame(got, st):
            if skip:
                return
            want = exp["rgb"]
            assert got.shape == want.shape, what
            assert np.array_equal(got, want), "%s: %d bytes differ from the oracle scene's, first at (y, x) %s" % (
                what, int((got != want).sum()), np.argwhere((got != want).any(axis=2))[:8].tolist())
            if st is not None:
                assert st["primary_hits"] == exp["primary_hits"], "%s: primary_hits %d, the oracle's %d" % (what, st["primary_hits"], exp["primary_hits"])

        if k == "render_rows":
            same_frame(*s.render_rows(ob["window"][0], ob["window"][1], device=dev, stats=True))
        elif k == "render_frame":
            same_frame(*s.render_frame(devices=(0, 0, 0), stats=True))
        elif k == "render_view_rows":
            same_frame(*s.render_view_rows(lib_view(rtx, v, (0, ob["window"][0], w, ob["window"][1])), device=dev, stats=True, **more))
        elif k == "render_view":
            res = s.render_view(lib_view(rtx, v, ob["rect"]), device=dev, stats=True, want_shade=ob["want_shade"], want_hits=ob["want_hits"], **more)
            same_frame(res[0], res[-1])
            if not skip and ob["want_shade"]:
                assert np.array_equal(res[1]["rgb8"], res[0]), what + ": the records' bytes are not the frame's"
                bad = np.argwhere((bits(res[1]["linear"]) != bits(exp["lin"])).any(axis=2))
                assert not len(bad), "%s: linear colours differ from the oracle scene's at (y, x) %s" % (what, bad[:8].tolist())
            if not skip and ob["want_hits"]:
                hits = res[2] if ob["want_shade"] else res[1]
                bad = np.argwhere(hits["prim"][:, :, 0] != exp["tri"])
                assert not len(bad), "%s: hit primitives differ from the oracle scene's at (y, x) %s" % (what, bad[:8].tolist())
        elif k == "trace_rays":
            hits = s.trace_rays(ob["origins"], ob["second"], device=dev, posed=ob["posed"], **order)
            if not skip:
                qs.check_hits(hits, exp["hits"], None, what)
                qs.check_normals(hits, exp["hits"], exp["tables"]["normals"], self.sc["kinds"], what)
        elif k == "occluded_rays":
            got = s.occluded_rays(ob["origins"], ob["second"], device=dev, posed=ob["posed"], **order)
            if not skip:
                assert np.array_equal(got, exp["occluded"]), "%s: occlusion differs at rays %s" % (what, np.nonzero(got != exp["occluded"])[0][:8].tolist())
        elif k == "shade_rays":
            res = s.shade_rays(ob["origins"], ob["second"], device=dev, want_hits=ob["want_hits"], **order, **more)
            shade = res[0] if ob["want_hits"] else res
            if not skip:
                bad = np.nonzero(shade.view(np.uint8).reshape(-1, 16) != exp["shade"].view(np.uint8).reshape(-1, 16))[0]
                assert not len(bad), "%s: shading differs from the composition at pixels %s" % (what, sorted(set(bad.tolist()))[:8])
                if ob["want_hits"]:
                    qs.check_hits(res[1], exp["hits"], None, what)
                    qs.check_normals(res[1], exp["hits"], exp["tables"]["normals"], self.sc["kinds"], what)
        else:                                                   # device-resident: same stream as the device poses
            t, stream = self.keep[ob["step"]], self.stream.cuda_stream
            out = t["out"]
            if k == "render_view_rows_device":
                s.render_view_rows_device(0, lib_view(rtx, v, (0, ob["window"][0], w, ob["window"][1])), out.data_ptr(), out.numel(), stream, **more)
            elif k == "render_view_device":
                s.render_view_device(0, lib_view(rtx, v, ob["rect"]), out.data_ptr(), t["shade"].data_ptr() if "shade" in t else None, None,
                                     stream, **more)
            else:
                s.shade_rays_device(0, len(ob["origins"]) // self.sc["kw"]["nb_ray"], t["origins"].data_ptr(), t["second"].data_ptr(),
                                    out.data_ptr(), None, stream, **order, **more)
            self.stream.synchronize()                           # the output is read: the first wait since the last one
            got = out.cpu().numpy()
            assert (got[-GUARD:] == 0xAA).all(), what + ": bytes behind the output were written"
            if skip:
                return
            if k == "shade_rays_device":
                a, b = got[:-GUARD].reshape(-1, 16), exp["shade"].view(np.uint8).reshape(-1, 16)
                bad = np.nonzero(a != b)[0]
                assert not len(bad), "%s: shading differs from the composition at pixels %s" % (what, sorted(set(bad.tolist()))[:8])
            else:
                same_frame(got[:-GUARD].reshape(exp["rgb"].shape), None)
                if "shade" in t:
                    rec = t["shade"].cpu().numpy()
                    assert (rec[-GUARD:] == 0xAA).all(), what + ": bytes behind the records were written"
                    rec = rec[:-GUARD].view(self.rtx.PIXEL_SHADE_DTYPE).reshape(exp["rgb"].shape[:2])
                    assert np.array_equal(rec["rgb8"], exp["rgb"]) and np.array_equal(bits(rec["linear"]), bits(exp["lin"])), what + ": records"

    # -- the sequence
    def run(self, expect):
        skipped = compared = 0
        for op in self.draw.log:
            what = "%s, seed %d, step %d (%s)\n%s\n" % (self.sc["name"], self.draw.seed, op["step"], sm.describe(op),
                                                        sm.log_text(self.draw.log, op["step"]))
            if op.get("refused"):
                self.refused(op, what)
                continue
            self.model.apply(op)
            kind = op["op"]
            if kind == "observe":
                exp = expect.observation(self.model, op)
                self.observe(op, exp, what)
                skipped += exp["skip"]
                compared += not exp["skip"]
            elif kind in sm.POSE_KINDS:
                self.pose(op)
                if op["read_back"]:
                    self.read_pose_back(op, what)
            elif kind == "skin":
                self.scene.skin(op["bones"], op["weights"], op["sphere_bone"])
                assert self.scene.skin_bound() == (op["bones"] is not None, self.model.max_bone()), what
            else:
                if kind == "resample":
                    self.scene.resample(op["table"])
                else:
                    self.scene.reseed(op["seed"], op["n_pairs"])
                if op["read_back"]:
                    self.read_table_back(what)
        self.torch.cuda.synchronize()
        return compared, skipped


@pytest.mark.parametrize("index", range(len(sm.FAMILY)), ids=sm.NAMES)
def test_a_sequence_matches_the_model(rtx, orc, samples_seeded, index):
    torch = pytest.importorskip("torch")
    assert torch.cuda.is_available(), "torch sees no GPU"
    t0 = time.perf_counter()
    table = np.ascontiguousarray(samples_seeded[:4096])
    n_devices = min(rtx.device_count(), 2)
    sc, draw = sm.draw_log(index, table, n_devices)
    expect = sm.Expect(orc, sc, draw.views)
    try:
        with sm.open_scene(rtx, sc, table) as scene:
            assert scene.pose_bound() == draw.model.bound
            compared, skipped = Runner(rtx, torch, scene, sc, draw, table).run(expect)
    finally:
        expect.close()
    print("%s: seed %d, %d steps, %d device(s), %d observations compared, %d outside the parity contract, %.2f s"
          % (sc["name"], draw.seed, len(draw.log), n_devices, compared, skipped, time.perf_counter() - t0))
    assert skipped * 4 <= compared + skipped, "more than a quarter of the observations lie outside the parity contract"
