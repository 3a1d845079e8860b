#!/usr/bin/env python3
"""Times posing on big_bunny's own 1920x1080 view: rtx_scene_pose_device and rtx_render_view_posed_device beside the way to
the same frame that needs no pose, a fresh scene per pose.

    pose_kernels           rtx_scene_pose_device alone on big_bunny + ground (4,969 records): the three pose kernels
    pose_kernels_1M        the same on the 1M-triangle soup + ground (--no-1m skips it)
    view_unposed           rtx_render_view_device, d_rgb only
    view_posed_identity    rtx_render_view_posed_device after the identity pose: the same frame through the pose's buffers
    posed_turn_K           the mesh turned by K of four angles about the vertical through its box centre:
                           rtx_scene_pose_device + rtx_render_view_posed_device, one event pair around both
    posed_view_turn_K      the posed view alone, the pose standing: the cost of walking the REFITTED tree
    fresh_turn_K           the same frame the old way: rtx_scene_create with the turned vertices + rtx_scene_upload (host wall
                           time, create_upload_ms) and rtx_render_view_device on the new scene (device time): a REBUILT tree

Device time between two events on the launch's stream, uncounted kernel forms.  The cases are interleaved: --repeats rounds
of one launch each after --warmup rounds; reported are the minimum, the median and the spread (max - min) / min.
view_posed_identity must give view_unposed's bytes and every posed_turn_K its fresh scene's, which the tool checks.
One JSON document on stdout, and in --out when given.

    python tools/pose_timing.py --out profiles/pose_timing.json

--pose-path --parent DIR --parent2 DIR [--bench]: in place of the above, the cost of every pose entry point on big_bunny +
ground in the 1920 x 1080 frame, of this build beside two separate builds of the parent commit under DIR.  The ten entry
points refitted, and rebuilt where they take the flag; a host call as the host's clock around it (wall) and as
RtxStats.total_ms (total), a device-resident call between two events on its stream.  Every build runs in a child process
of its own, --rounds times, who goes first rotating; in a child --repeats rounds of one call per case follow --warmup
rounds.  Per case: the pooled samples' summary per build, and whether this build's median is no further from the nearer
parent's than the two parents' medians are apart.  --bench adds bench.py --gpus 1 --steps 20 --warmup 3 of the three.

    python tools/pose_timing.py --pose-path --parent build_ab/parent --parent2 build_ab/parent2 --bench --out run_1.json
"""
import argparse
import importlib
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TURN_DEGREES = (25.0, 115.0, 205.0, 295.0)


def turned(tris, n_mesh, degrees):
    """the first n_mesh triangles turned about the vertical through their box centre, float32"""
    out = np.array(tris, np.float64).reshape(-1, 3, 3)
    mesh = out[:n_mesh]
    c = 0.5 * (mesh.reshape(-1, 3).min(axis=0) + mesh.reshape(-1, 3).max(axis=0))
    a = np.deg2rad(degrees)
    x, z = mesh[..., 0] - c[0], mesh[..., 2] - c[2]
    mesh[..., 0], mesh[..., 2] = c[0] + np.cos(a) * x + np.sin(a) * z, c[2] - np.sin(a) * x + np.cos(a) * z
    return np.ascontiguousarray(out.reshape(-1, 9).astype(np.float32))


def summary(v):
    return {"min_ms": round(min(v), 5), "median_ms": round(float(np.median(v)), 5), "spread": round((max(v) - min(v)) / min(v), 4)}


def pose_calls(root, warmup, repeats):
    """--pose-path's child: the build under `root` (its binding and its library) -> the samples of every case"""
    import torch  # before librtx.so: one HIP runtime per process (tests/conftest.py)
    sys.path.insert(0, root)
    rtx = importlib.import_module("ray-tracer-rust_amd")
    tris, rgb = rtx.default_primitives([os.path.join(root, "models", "big_bunny.obj")])
    n_mesh = len(tris) - 1
    sc = rtx.Scene(rtx.DEFAULT_WIDTH, rtx.DEFAULT_HEIGHT, tris, rgb, rtx.gen_samples())
    sc.upload(0)
    v = turned(tris, n_mesh, TURN_DEGREES[0])
    mesh = np.array(tris, np.float64).reshape(-1, 3, 3)[:n_mesh].reshape(-1, 3)
    c, a = 0.5 * (mesh.min(axis=0) + mesh.max(axis=0)), np.deg2rad(TURN_DEGREES[0])
    lin = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
    turn = np.concatenate([lin, (c - lin @ c).reshape(3, 1)], axis=1).reshape(12)
    moves = np.stack([np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0.0]), turn]).astype(np.float32)
    group = np.full(len(tris), 0xFFFFFFFF, np.uint32)      # the mesh follows move 1, the ground none
    group[:n_mesh] = 1
    bones = np.full((len(tris), 3, 4), 0xFFFFFFFF, np.uint32)
    bones[:n_mesh, :, 0], bones[:n_mesh, :, 1] = 0, 1
    weights = np.zeros((len(tris), 3, 4), np.float32)
    weights[:n_mesh, :, 0], weights[:n_mesh, :, 1] = 0.25, 0.75
    sc.skin(bones, weights)
    stream = torch.cuda.Stream(device="cuda:0")
    s = stream.cuda_stream
    dev = {k: torch.from_numpy(x.view(np.int32) if x.dtype == np.uint32 else x).to("cuda:0") for k, x in
           dict(v=v, rgb=np.ascontiguousarray(rgb, np.float32), moves=moves, group=group).items()}
    torch.cuda.synchronize()
    d = {k: t.data_ptr() for k, t in dev.items()}
    host = {"pose": lambda r, **kw: (sc.pose_rebuilt if r else sc.pose)(v, **kw),
            "pose_prims": lambda r, **kw: sc.pose_prims(v, rgb=rgb, rebuilt=r, **kw),
            "pose_moved": lambda r, **kw: sc.pose_moved(moves, group, rebuilt=r, **kw),
            "pose_skinned": lambda r, **kw: sc.pose_skinned(moves, rebuilt=r, **kw)}
    device = {"pose_device": lambda r: (sc.pose_rebuilt_device if r else sc.pose_device)(0, d["v"], None, s),
              "pose_prims_device": lambda r: sc.pose_prims_device(0, d["v"], d_rgb_ptr=d["rgb"], rebuilt=r, stream=s),
              "pose_moved_device": lambda r: sc.pose_moved_device(0, 2, d["moves"], d["group"], rebuilt=r, stream=s),
              "pose_skinned_device": lambda r: sc.pose_skinned_device(0, 2, d["moves"], rebuilt=r, stream=s)}
    ms = {}
    for i in range(warmup + repeats):
        keep = ms if i >= warmup else {}
        for r in (False, True):
            tree = "rebuilt" if r else "refitted"
            for name, f in host.items():
                stream.synchronize()
                t0 = time.perf_counter()
                f(r)
                keep.setdefault("%s_%s_wall" % (name, tree), []).append(1e3 * (time.perf_counter() - t0))
                keep.setdefault("%s_%s_total" % (name, tree), []).append(f(r, stats=True)["total_ms"])
            for name, f in device.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                f(r)
                e1.record(stream)
                e1.synchronize()
                keep.setdefault("%s_%s" % (name, tree), []).append(e0.elapsed_time(e1))
    sc.close()
    return {"lib": rtx.rtx.LIB_PATH, "ms": ms}


def pose_path(args, roots):
    """--pose-path: pose_calls of every build in a child process each, --rounds times -> per case the summaries and the verdict"""
    pooled = {who: {} for who, _ in roots}
    for k in range(args.rounds):
        for who, root in roots[k % len(roots):] + roots[:k % len(roots)]:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--pose-calls", root, "--repeats", str(args.repeats), "--warmup",
                                str(args.warmup)], capture_output=True, text=True, timeout=600)
            if r.returncode != 0:
                raise SystemExit("child for %s failed (%d):\n%s" % (who, r.returncode, (r.stdout + r.stderr)[-3000:]))
            child = json.loads(r.stdout.splitlines()[-1])
            assert child["lib"].startswith(root + os.sep), child["lib"]
            for case, v in child["ms"].items():
                pooled[who].setdefault(case, []).extend(v)
            print("round %d, %s: done" % (k, who), file=sys.stderr, flush=True)
    out = {}
    for case in pooled["this"]:
        med = {who: float(np.median(v[case])) for who, v in pooled.items()}
        out[case] = {who: summary(v[case]) for who, v in pooled.items()}
        between = abs(med["parent"] - med["parent2"])
        nearer = min(("parent", "parent2"), key=lambda who: abs(med["this"] - med[who]))
        out[case].update(parents_apart_ms=round(between, 5), this_minus_nearer_parent_ms=round(med["this"] - med[nearer], 5),
                         within=bool(abs(med["this"] - med[nearer]) <= between))
    return out


def bench_line(root):
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--steps", "20", "--warmup", "3"],
                       capture_output=True, text=True, cwd=root, timeout=900)
    if r.returncode != 0:
        raise SystemExit("bench.py under %s failed (%d):\n%s" % (root, r.returncode, (r.stdout + r.stderr)[-3000:]))
    line = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    return {k: v for k, v in line.items() if not isinstance(v, (dict, list))}      # (the scalars)


def pose_path_doc(args):
    if not (args.parent and args.parent2):
        raise SystemExit("--pose-path needs --parent and --parent2: two builds of the parent commit")
    roots = [(who, os.path.abspath(root)) for who, root in (("parent", args.parent), ("this", ROOT), ("parent2", args.parent2))]
    doc = {"frame": [1920, 1080], "rounds": args.rounds, "repeats": args.repeats, "warmup": args.warmup, "pose_calls": pose_path(args, roots)}
    doc["not_within"] = sorted(case for case, row in doc["pose_calls"].items() if not row["within"])
    if args.bench:
        lines = {who: [] for who, _ in roots}
        for k in range(args.rounds):
            for who, root in roots[::-1] if k % 2 else roots:
                lines[who].append(bench_line(root))
        doc["bench"] = {"command": "bench.py --gpus 1 --steps 20 --warmup 3", **lines}
    return doc


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--no-1m", action="store_true")
    ap.add_argument("--pose-path", action="store_true", help="the ten entry points of this build beside two builds of the parent")
    ap.add_argument("--pose-calls", default=None, metavar="ROOT", help="--pose-path's child: the pose calls of the build under ROOT")
    ap.add_argument("--parent", default=None, help="--pose-path: the parent commit's tree, built")
    ap.add_argument("--parent2", default=None, help="--pose-path: a second copy of it")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--bench", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.pose_calls:
        print(json.dumps(pose_calls(os.path.abspath(args.pose_calls), args.warmup, args.repeats)))
        return
    if args.pose_path:
        text = json.dumps(pose_path_doc(args), indent=1)
        print(text)
        if args.out:
            with open(args.out, "w") as f:
                f.write(text + "\n")
        return

    import torch  # before librtx.so: one HIP runtime per process (tests/conftest.py)
    sys.path.insert(0, ROOT)
    rtx = importlib.import_module("ray-tracer-rust_amd")
    if rtx.device_count() < 1 or not torch.cuda.is_available():
        raise SystemExit("no HIP device: rendering has no CPU fallback")
    width, height = rtx.DEFAULT_WIDTH, rtx.DEFAULT_HEIGHT
    samples = rtx.gen_samples()
    tris, rgb_of = rtx.default_primitives([os.path.join(ROOT, "models", "big_bunny.obj")])
    n_mesh = len(tris) - 1
    scene = rtx.Scene(width, height, tris, rgb_of, samples)
    n = width * height
    poses = [turned(tris, n_mesh, d) for d in TURN_DEGREES]
    assert all(np.abs(p).max() <= scene.pose_bound() for p in poses)
    stream = torch.cuda.Stream(device="cuda:0")
    with torch.cuda.stream(stream):
        s = stream.cuda_stream
        own = scene.own_view()
        buf = {}

        def out(name):
            buf[name] = torch.zeros(n * 3, dtype=torch.uint8, device="cuda:0")
            return buf[name].data_ptr()

        d_identity = torch.from_numpy(np.ascontiguousarray(tris)).to("cuda:0")
        d_poses = [torch.from_numpy(p).to("cuda:0") for p in poses]
        stream.synchronize()

        def timed(launch):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            launch()
            e1.record(stream)
            e1.synchronize()
            return e0.elapsed_time(e1)

        def posed_view(d_pose, p):
            scene.pose_device(0, d_pose.data_ptr(), None, s)
            scene.render_view_device(0, own, p, None, None, s, posed=True)

        def identity_view(p):
            scene.render_view_device(0, own, p, None, None, s, posed=True)

        names = ["pose_kernels", "view_unposed", "view_posed_identity"]
        names += ["posed_turn_%d" % k for k in range(4)] + ["posed_view_turn_%d" % k for k in range(4)] + ["fresh_turn_%d" % k for k in range(4)]
        ms = {k: [] for k in names}
        create_ms = {k: [] for k in range(4)}
        for name in ("view_unposed", "view_posed_identity"):
            out(name)
        for k in range(4):
            out("posed_turn_%d" % k)
            out("posed_view_turn_%d" % k)
            out("fresh_turn_%d" % k)
        for i in range(args.warmup + args.repeats):
            keep = i >= args.warmup
            t = timed(lambda: scene.pose_device(0, d_identity.data_ptr(), None, s))
            ms["pose_kernels"] += [t] if keep else []
            t = timed(lambda: scene.render_view_device(0, own, buf["view_unposed"].data_ptr(), None, None, s))
            ms["view_unposed"] += [t] if keep else []
            t = timed(lambda: identity_view(buf["view_posed_identity"].data_ptr()))
            ms["view_posed_identity"] += [t] if keep else []
            for k in range(4):
                t = timed(lambda: posed_view(d_poses[k], buf["posed_turn_%d" % k].data_ptr()))
                ms["posed_turn_%d" % k] += [t] if keep else []
                t = timed(lambda: identity_view(buf["posed_view_turn_%d" % k].data_ptr()))       # the pose of turn k stands
                ms["posed_view_turn_%d" % k] += [t] if keep else []
                name = "fresh_turn_%d" % k
                t0 = time.perf_counter()
                fresh = rtx.Scene(width, height, poses[k], rgb_of, samples)
                fresh.upload(0)
                t1 = time.perf_counter()
                fresh.render_view_device(0, own, buf[name].data_ptr(), None, None, s)      # (first launch on a new scene)
                stream.synchronize()
                t = timed(lambda: fresh.render_view_device(0, own, buf[name].data_ptr(), None, None, s))
                fresh.close()
                if keep:
                    ms[name].append(t)
                    create_ms[k].append((t1 - t0) * 1e3)
        frame = buf["view_unposed"].cpu().numpy()
        same = {"pose_kernels": True, "view_unposed": True,
                "view_posed_identity": bool(np.array_equal(buf["view_posed_identity"].cpu().numpy(), frame))}
        for k in range(4):
            fresh = buf["fresh_turn_%d" % k].cpu().numpy()
            same["fresh_turn_%d" % k] = bool((fresh != frame).any())                        # another pose: another frame
            same["posed_turn_%d" % k] = bool(np.array_equal(buf["posed_turn_%d" % k].cpu().numpy(), fresh))
            same["posed_view_turn_%d" % k] = bool(np.array_equal(buf["posed_view_turn_%d" % k].cpu().numpy(), fresh))
        big = None
        if not args.no_1m:
            t0 = time.perf_counter()
            bt, brgb = rtx.synthetic_primitives(1000000)
            soup = rtx.Scene(width, height, bt, brgb, samples, reference_tree=rtx.REFTREE_NEVER, tie_rank=None)
            soup.upload(0)
            t1 = time.perf_counter()
            d_big = torch.from_numpy(np.ascontiguousarray(bt)).to("cuda:0")
            stream.synchronize()
            v = [timed(lambda: soup.pose_device(0, d_big.data_ptr(), None, s)) for _ in range(args.warmup + args.repeats)][args.warmup:]
            info = soup.info()
            big = {"case": "pose_kernels_1M", "min_ms": round(min(v), 4), "median_ms": round(float(np.median(v)), 4),
                   "spread": round((max(v) - min(v)) / min(v), 4), "records": info["n_tris"], "nodes": info["n_nodes"],
                   "depth": info["depth"], "create_upload_ms": round((t1 - t0) * 1e3, 1)}
            soup.close()
    doc = {"scene": "big_bunny.obj + ground, %dx%d, default camera, rgb only" % (width, height), "device": torch.cuda.get_device_name(0),
           "repeats": args.repeats, "warmup": args.warmup, "pixels": n, "turn_degrees": list(TURN_DEGREES), "cases": []}
    for name, v in ms.items():
        row = {"case": name, "min_ms": round(min(v), 4), "median_ms": round(float(np.median(v)), 4),
               "spread": round((max(v) - min(v)) / min(v), 4), "bytes_as_expected": same[name]}
        if name.startswith("fresh_turn_"):
            c = create_ms[int(name.rsplit("_", 1)[1])]
            row["create_upload_ms"] = {"min": round(min(c), 2), "median": round(float(np.median(c)), 2)}
        doc["cases"].append(row)
        print("%-22s min %9.4f ms  median %9.4f ms  spread %.3f  bytes as expected: %s" %
              (name, row["min_ms"], row["median_ms"], row["spread"], same[name]), file=sys.stderr)
    if big:
        doc["cases"].append(big)
        print("%-22s min %9.4f ms  median %9.4f ms  spread %.3f" % (big["case"], big["min_ms"], big["median_ms"], big["spread"]), file=sys.stderr)
    by = {r["case"]: r for r in doc["cases"]}
    doc["turns"] = []
    for k in range(4):
        posed, fresh, walk = by["posed_turn_%d" % k], by["fresh_turn_%d" % k], by["posed_view_turn_%d" % k]
        fresh_total = fresh["create_upload_ms"]["median"] + fresh["median_ms"]
        doc["turns"].append({"degrees": TURN_DEGREES[k], "pose_and_posed_view_ms": posed["median_ms"],
                             "fresh_create_upload_and_view_ms": round(fresh_total, 3),
                             "posed_is_sooner": bool(posed["median_ms"] < fresh_total),
                             "refitted_over_rebuilt_view": round(walk["median_ms"] / fresh["median_ms"], 4)})
    identity, plain = by["view_posed_identity"], by["view_unposed"]
    noise = max(identity["spread"] * identity["min_ms"], plain["spread"] * plain["min_ms"])
    doc["identity"] = {"what": "view_posed_identity median - view_unposed median against the run-to-run spread observed",
                       "excess_ms": round(identity["median_ms"] - plain["median_ms"], 4), "spread_observed_ms": round(noise, 4),
                       "within_spread": bool(identity["median_ms"] - plain["median_ms"] <= noise)}
    text = json.dumps(doc, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    scene.close()
    if not all(same.values()):
        raise SystemExit("a case's bytes are not what they should be")


if __name__ == "__main__":
    main()
