#!/usr/bin/env python3
"""Times a pose through the render pipeline on big_bunny's own 1920x1080 view: rtx_render_view_rows_posed_device beside its
unposed twin, beside the one-wavefront-per-tile posed renderer, and beside a fresh scene per pose.

  (a) rows_unposed / rows_posed_identity   rtx_render_view_rows_device and, after the identity pose,
                           rtx_render_view_rows_posed_device: the same kernels, other pointers
  (b) per turn K of four angles about the vertical through the mesh's box centre, one event pair around each:
      pose_rows_turn_K     rtx_scene_pose_device + rtx_render_view_rows_posed_device (the pose kernels, the plane kernel,
                           the aim kernels — a new pose always aims again — and the pipeline)
      pose_view_turn_K     rtx_scene_pose_device + rtx_render_view_posed_device: what an animation paid per frame before
      rows_posed_turn_K    the posed rows alone, the pose and its aimed stream standing: walking the REFITTED tree
      fresh_rows_turn_K    rtx_render_view_rows_device on a scene created with the turned vertices: a REBUILT tree
                           (rtx_scene_create + rtx_scene_upload: host wall time, create_upload_ms)
      every frame is compared byte for byte with the fresh scene's
  (c) --pose-only          the pose kernels alone (rtx_scene_pose_device, which now ends with the plane kernel) on big_bunny
                           and on the 1M-triangle soup + ground, of the build under --root; --parent DIR alternates
                           --rounds child processes of this build and of the build under DIR
  (d) --bench DIR          bench.py --gpus 1 --steps 20 --warmup 3 of the build under DIR and of this one, alternated
                           --rounds times, each a child process

Device time between two events on the launch's stream, uncounted kernel forms.  (a) and (b) are interleaved: --repeats rounds
of one launch each after --warmup rounds; reported are the minimum, the median and the spread (max - min) / min.
One JSON document on stdout, and in --out when given.

    python tools/posed_rows_timing.py --parent ../parent --bench ../parent --out profiles/posed_rows_timing.json
"""
import argparse
import importlib
import json
import os
import subprocess
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TURN_DEGREES = (25.0, 115.0, 205.0, 295.0)         # tests/pose_sets.py: TURNTABLE_DEGREES


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
    return {"min_ms": round(min(v), 4), "median_ms": round(float(np.median(v)), 4), "spread": round((max(v) - min(v)) / min(v), 4)}


def load(root):
    import torch  # before librtx.so: one HIP runtime per process (tests/conftest.py)
    sys.path.insert(0, root)
    rtx = importlib.import_module("ray-tracer-rust_amd")
    if rtx.device_count() < 1 or not torch.cuda.is_available():
        raise SystemExit("no HIP device: rendering has no CPU fallback")
    return torch, rtx


def pose_only(args):
    """(c), one build: the pose kernels alone on big_bunny + ground and on the 1M soup + ground"""
    torch, rtx = load(args.root)
    samples = rtx.gen_samples()
    stream = torch.cuda.Stream(device="cuda:0")
    out = {"root": os.path.abspath(args.root), "cases": []}
    with torch.cuda.stream(stream):
        s = stream.cuda_stream

        def timed(launch):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            launch()
            e1.record(stream)
            e1.synchronize()
            return e0.elapsed_time(e1)

        tris, rgb = rtx.default_primitives([os.path.join(args.root, "models", "big_bunny.obj")])
        sets = [("pose_kernels", tris, rgb, {})]
        if not args.no_1m:
            bt, brgb = rtx.synthetic_primitives(1000000)
            sets.append(("pose_kernels_1M", bt, brgb, dict(reference_tree=rtx.REFTREE_NEVER, tie_rank=None)))
        for name, t, c, kw in sets:
            scene = rtx.Scene(rtx.DEFAULT_WIDTH, rtx.DEFAULT_HEIGHT, t, c, samples, **kw)
            scene.upload(0)
            d_pose = torch.from_numpy(np.ascontiguousarray(t)).to("cuda:0")
            stream.synchronize()
            v = [timed(lambda: scene.pose_device(0, d_pose.data_ptr(), None, s)) for _ in range(args.warmup + args.repeats)][args.warmup:]
            out["cases"].append(dict(summary(v), case=name, records=scene.info()["n_tris"], n_global=scene.info()["n_global"]))
            scene.close()
    print(json.dumps(out))


def child(argv, cwd=None):
    r = subprocess.run([sys.executable] + argv, capture_output=True, text=True, cwd=cwd, timeout=900)
    if r.returncode != 0:
        raise SystemExit("child %s failed (%d):\n%s" % (argv, r.returncode, (r.stdout + r.stderr)[-3000:]))
    return json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--root", default=HERE, help="the build --pose-only measures")
    ap.add_argument("--pose-only", action="store_true")
    ap.add_argument("--no-1m", action="store_true")
    ap.add_argument("--parent", default=None, help="(c): the parent commit's tree, built")
    ap.add_argument("--bench", default=None, help="(d): the parent commit's tree, built")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.pose_only:
        return pose_only(args)

    torch, rtx = load(HERE)
    width, height = rtx.DEFAULT_WIDTH, rtx.DEFAULT_HEIGHT
    samples = rtx.gen_samples()
    tris, rgb_of = rtx.default_primitives([os.path.join(HERE, "models", "big_bunny.obj")])
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
            return buf[name]

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

        def rows(sc, name, posed):
            sc.render_view_rows_device(0, own, buf[name].data_ptr(), n * 3, s, posed=posed)

        kinds = ("pose_rows_turn_%d", "pose_view_turn_%d", "rows_posed_turn_%d", "fresh_rows_turn_%d")
        names = ["rows_unposed", "rows_posed_identity"] + [k % i for k in kinds for i in range(4)]
        ms = {k: [] for k in names}
        create_ms = {k: [] for k in range(4)}
        for name in names:
            out(name)
        for i in range(args.warmup + args.repeats):
            keep = i >= args.warmup

            def add(name, t):
                if keep:
                    ms[name].append(t)

            scene.pose_device(0, d_identity.data_ptr(), None, s)
            rows(scene, "rows_posed_identity", True)                   # (aims over the new pose: not timed)
            for _ in range(2):                                         # interleaved, either order
                add("rows_unposed", timed(lambda: rows(scene, "rows_unposed", False)))
                add("rows_posed_identity", timed(lambda: rows(scene, "rows_posed_identity", True)))
            for k in range(4):
                def pose_rows():
                    scene.pose_device(0, d_poses[k].data_ptr(), None, s)
                    rows(scene, "pose_rows_turn_%d" % k, True)

                def pose_view():
                    scene.pose_device(0, d_poses[k].data_ptr(), None, s)
                    scene.render_view_device(0, own, buf["pose_view_turn_%d" % k].data_ptr(), None, None, s, posed=True)

                add("pose_view_turn_%d" % k, timed(pose_view))
                add("pose_rows_turn_%d" % k, timed(pose_rows))
                add("rows_posed_turn_%d" % k, timed(lambda: rows(scene, "rows_posed_turn_%d" % k, True)))    # pose k and its aim stand
                name = "fresh_rows_turn_%d" % k
                t0 = time.perf_counter()
                fresh = rtx.Scene(width, height, poses[k], rgb_of, samples)
                fresh.upload(0)
                t1 = time.perf_counter()
                rows(fresh, name, False)                                # (first launch on a new scene, and its aim)
                stream.synchronize()
                add(name, timed(lambda: rows(fresh, name, False)))
                fresh.close()
                if keep:
                    create_ms[k].append((t1 - t0) * 1e3)
        frame = buf["rows_unposed"].cpu().numpy()
        same = {"rows_unposed": True, "rows_posed_identity": bool(np.array_equal(buf["rows_posed_identity"].cpu().numpy(), frame))}
        for k in range(4):
            fresh = buf["fresh_rows_turn_%d" % k].cpu().numpy()
            same["fresh_rows_turn_%d" % k] = bool((fresh != frame).any())                     # another pose: another frame
            for kind in kinds[:3]:
                same[kind % k] = bool(np.array_equal(buf[kind % k].cpu().numpy(), fresh))
    doc = {"scene": "big_bunny.obj + ground, %dx%d, default camera, rgb only" % (width, height), "device": torch.cuda.get_device_name(0),
           "repeats": args.repeats, "warmup": args.warmup, "pixels": n, "turn_degrees": list(TURN_DEGREES), "cases": []}
    for name, v in ms.items():
        row = dict(summary(v), case=name, bytes_as_expected=same[name])
        if name.startswith("fresh_rows_turn_"):
            c = create_ms[int(name.rsplit("_", 1)[1])]
            row["create_upload_ms"] = {"min": round(min(c), 2), "median": round(float(np.median(c)), 2)}
        doc["cases"].append(row)
        print("%-22s min %9.4f ms  median %9.4f ms  spread %.3f  bytes as expected: %s" %
              (name, row["min_ms"], row["median_ms"], row["spread"], same[name]), file=sys.stderr)
    by = {r["case"]: r for r in doc["cases"]}
    identity, plain = by["rows_posed_identity"], by["rows_unposed"]
    noise = max(identity["spread"] * identity["min_ms"], plain["spread"] * plain["min_ms"])
    doc["identity"] = {"what": "rows_posed_identity median - rows_unposed median against the run-to-run spread observed",
                       "excess_ms": round(identity["median_ms"] - plain["median_ms"], 4), "spread_observed_ms": round(noise, 4),
                       "within_spread": bool(abs(identity["median_ms"] - plain["median_ms"]) <= noise)}
    doc["turns"] = []
    for k in range(4):
        pr, pv, walk, fresh = (by[kind % k] for kind in kinds)
        doc["turns"].append({"degrees": TURN_DEGREES[k], "pose_and_posed_rows_ms": pr["median_ms"], "pose_and_posed_view_ms": pv["median_ms"],
                             "posed_view_over_posed_rows": round(pv["median_ms"] / pr["median_ms"], 3),
                             "refitted_over_rebuilt_rows": round(walk["median_ms"] / fresh["median_ms"], 4),
                             "fresh_create_upload_ms": fresh["create_upload_ms"]["median"]})
    scene.close()
    if args.parent:                                                     # (c)
        runs = {"this": [], "parent": []}
        for _ in range(args.rounds):
            for who, root in (("parent", args.parent), ("this", HERE)):
                argv = [os.path.abspath(__file__), "--pose-only", "--root", os.path.abspath(root), "--repeats", str(args.repeats),
                        "--warmup", str(args.warmup)] + (["--no-1m"] if args.no_1m else [])
                runs[who].append(child(argv)["cases"])
        doc["pose_kernels"] = []
        for idx, case in enumerate(c["case"] for c in runs["this"][0]):
            row = {"case": case, "records": runs["this"][0][idx]["records"], "n_global": runs["this"][0][idx]["n_global"]}
            for who in ("parent", "this"):
                med = [r[idx]["median_ms"] for r in runs[who]]
                row[who] = {"median_ms_per_round": med, "median_ms": round(float(np.median(med)), 4), "min_ms": min(r[idx]["min_ms"] for r in runs[who]),
                            "spread_within_a_round": max(r[idx]["spread"] for r in runs[who])}
            row["this_minus_parent_ms"] = round(row["this"]["median_ms"] - row["parent"]["median_ms"], 4)
            doc["pose_kernels"].append(row)
    if args.bench:                                                      # (d)
        lines = {"parent": [], "this": []}
        for _ in range(args.rounds):
            for who, root in (("parent", os.path.abspath(args.bench)), ("this", HERE)):
                line = child([os.path.join(root, "bench.py"), "--gpus", "1", "--steps", "20", "--warmup", "3"], cwd=root)
                lines[who].append({k: v for k, v in line.items() if not isinstance(v, (dict, list))})      # (the scalars)
        doc["bench"] = {"command": "bench.py --gpus 1 --steps 20 --warmup 3", "parent": lines["parent"], "this": lines["this"]}
    text = json.dumps(doc, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    if not all(same.values()):
        raise SystemExit("a case's bytes are not what they should be")


if __name__ == "__main__":
    main()
