#!/usr/bin/env python3
"""Times a pose whose tree is rebuilt on the device (rtx_scene_pose_rebuilt_device) beside the refitting pose
(rtx_scene_pose_device) and beside a fresh scene per pose, 1920x1080, own camera, RGB only.

  (1) the kernels alone, interleaved:
      refit_kernels / rebuild_kernels       rtx_scene_pose_device / rtx_scene_pose_rebuilt_device (the key kernel, the sort,
                                            the record kernel, the refit; both end with the plane kernel) on big_bunny +
                                            ground, and (..._1M) on the 1M-triangle soup + ground
  (2) per pose — four turns of big_bunny about the vertical through its box centre, and SCATTER: the 20,000-triangle soup
      + ground re-drawn with another seed — one event pair around each:
      rebuilt_pose_rows_P    rtx_scene_pose_rebuilt_device + rtx_render_view_rows_posed_device
      refit_pose_rows_P      rtx_scene_pose_device + rtx_render_view_rows_posed_device
      rebuilt_rows_P         the posed rows alone over the rebuilt tree, the pose and its aimed stream standing
      refit_rows_P           the same over the refitted tree
      fresh_rows_P           rtx_render_view_rows_device on a scene created with the posed vertices: the host's SAH tree
                             (rtx_scene_create + rtx_scene_upload: host wall time, create_upload_ms)
      every frame is compared byte for byte with the fresh scene's
  (3) --bench DIR            bench.py --gpus 1 --steps 20 --warmup 3 of the build under DIR and of this one, alternated
                             --rounds times, each a child process

Device time between two events on the launch's stream, uncounted kernel forms; --repeats interleaved rounds after --warmup
rounds; reported are the minimum, the median and the spread (max - min) / min.  One JSON document on stdout, and in --out.

    python tools/pose_rebuild_timing.py --bench ../parent --out profiles/pose_rebuild_timing.json
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
SCATTER_N, SCATTER_SEED = 20000, 4242              # tests/rebuild_sets.py


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
    ap.add_argument("--no-1m", action="store_true")
    ap.add_argument("--bench", default=None, help="(3): the parent commit's tree, built")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch  # before librtx.so: one HIP runtime per process (tests/conftest.py)
    sys.path.insert(0, HERE)
    rtx = importlib.import_module("ray-tracer-rust_amd")
    if rtx.device_count() < 1 or not torch.cuda.is_available():
        raise SystemExit("no HIP device: rendering has no CPU fallback")
    width, height = rtx.DEFAULT_WIDTH, rtx.DEFAULT_HEIGHT
    n = width * height
    samples = rtx.gen_samples()
    stream = torch.cuda.Stream(device="cuda:0")
    doc = {"scene": "%dx%d, default camera, rgb only" % (width, height), "device": torch.cuda.get_device_name(0),
           "repeats": args.repeats, "warmup": args.warmup, "kernels": [], "cases": [], "poses": []}
    same = {}
    with torch.cuda.stream(stream):
        s = stream.cuda_stream

        def timed(launch):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            launch()
            e1.record(stream)
            e1.synchronize()
            return e0.elapsed_time(e1)

        tris, rgb = rtx.default_primitives([os.path.join(HERE, "models", "big_bunny.obj")])
        never = dict(reference_tree=rtx.REFTREE_NEVER, tie_rank=None)
        # ---- (1) the kernels alone
        sets = [("", tris, rgb, {})]
        if not args.no_1m:
            bt, brgb = rtx.synthetic_primitives(1000000)
            sets.append(("_1M", bt, brgb, never))
        for tag, t, c, kw in sets:
            scene = rtx.Scene(width, height, t, c, samples, **kw)
            scene.upload(0)
            d_pose = torch.from_numpy(np.ascontiguousarray(t)).to("cuda:0")
            stream.synchronize()
            ms = {"refit_kernels" + tag: [], "rebuild_kernels" + tag: []}
            for i in range(args.warmup + args.repeats):
                for name, call in (("refit_kernels" + tag, scene.pose_device), ("rebuild_kernels" + tag, scene.pose_rebuilt_device)):
                    v = timed(lambda: call(0, d_pose.data_ptr(), None, s))
                    if i >= args.warmup:
                        ms[name].append(v)
            for name, v in ms.items():
                doc["kernels"].append(dict(summary(v), case=name, records=scene.info()["n_tris"], nodes=scene.info()["n_nodes"],
                                           rebuilt_nodes=scene.rebuilt_counts()))
                print("%-24s min %9.4f ms  median %9.4f ms  spread %.3f" % (name, min(v), float(np.median(v)), (max(v) - min(v)) / min(v)),
                      file=sys.stderr)
            scene.close()
            del d_pose

        # ---- (2) per pose
        soup, srgb = rtx.synthetic_primitives(SCATTER_N)
        redrawn = np.ascontiguousarray(np.concatenate([rtx.synthetic_mesh(SCATTER_N, seed=SCATTER_SEED), soup[-1:]]))
        cases = [("turn_%d" % k, tris, rgb, turned(tris, len(tris) - 1, d), {}) for k, d in enumerate(TURN_DEGREES)]
        cases.append(("scatter", soup, srgb, redrawn, never))
        scenes = {}
        kinds = ("rebuilt_pose_rows_%s", "refit_pose_rows_%s", "rebuilt_rows_%s", "refit_rows_%s", "fresh_rows_%s")
        ms, create_ms, buf = {}, {}, {}
        for name, t, c, pose, kw in cases:
            key = id(t)
            if key not in scenes:
                scenes[key] = rtx.Scene(width, height, t, c, samples, **kw)
                scenes[key].upload(0)
                assert np.abs(pose).max() <= scenes[key].pose_bound()
            for kind in kinds:
                ms[kind % name] = []
                buf[kind % name] = torch.zeros(n * 3, dtype=torch.uint8, device="cuda:0")
            create_ms[name] = []
        d_poses = {name: torch.from_numpy(pose).to("cuda:0") for name, _, _, pose, _ in cases}
        stream.synchronize()
        for i in range(args.warmup + args.repeats):
            keep = i >= args.warmup
            for name, t, c, pose, kw in cases:
                scene = scenes[id(t)]
                own = scene.own_view()

                def rows(sc, which, posed):
                    sc.render_view_rows_device(0, own, buf[which].data_ptr(), n * 3, s, posed=posed)

                def add(which, v):
                    if keep:
                        ms[which].append(v)

                def rebuilt_pose_rows():
                    scene.pose_rebuilt_device(0, d_poses[name].data_ptr(), None, s)
                    rows(scene, "rebuilt_pose_rows_" + name, True)

                def refit_pose_rows():
                    scene.pose_device(0, d_poses[name].data_ptr(), None, s)
                    rows(scene, "refit_pose_rows_" + name, True)

                add("refit_pose_rows_" + name, timed(refit_pose_rows))
                add("refit_rows_" + name, timed(lambda: rows(scene, "refit_rows_" + name, True)))          # pose and aim stand
                add("rebuilt_pose_rows_" + name, timed(rebuilt_pose_rows))
                add("rebuilt_rows_" + name, timed(lambda: rows(scene, "rebuilt_rows_" + name, True)))
                t0 = time.perf_counter()
                fresh = rtx.Scene(width, height, pose, c, samples, **kw)
                fresh.upload(0)
                t1 = time.perf_counter()
                rows(fresh, "fresh_rows_" + name, False)                # (first launch on a new scene, and its aim)
                stream.synchronize()
                add("fresh_rows_" + name, timed(lambda: rows(fresh, "fresh_rows_" + name, False)))
                fresh.close()
                if keep:
                    create_ms[name].append((t1 - t0) * 1e3)
        for name, t, c, pose, kw in cases:
            fresh = buf["fresh_rows_" + name].cpu().numpy()
            same["fresh_rows_" + name] = bool(fresh.any())
            for kind in kinds[:4]:
                same[kind % name] = bool(np.array_equal(buf[kind % name].cpu().numpy(), fresh))
        for sc in scenes.values():
            sc.close()
    for which, v in ms.items():
        row = dict(summary(v), case=which, bytes_as_expected=same[which])
        doc["cases"].append(row)
        print("%-28s min %9.4f ms  median %9.4f ms  spread %.3f  bytes as expected: %s" %
              (which, row["min_ms"], row["median_ms"], row["spread"], same[which]), file=sys.stderr)
    by = {r["case"]: r for r in doc["cases"]}
    for name, t, c, pose, kw in cases:
        rp, fp, rr, fr, fresh = (by[kind % name]["median_ms"] for kind in kinds)
        cu = create_ms[name]
        doc["poses"].append({"pose": name, "triangles": len(t), "rebuilt_pose_and_rows_ms": rp, "refit_pose_and_rows_ms": fp,
                             "rebuilt_rows_ms": rr, "refit_rows_ms": fr, "fresh_rows_ms": fresh,
                             "fresh_create_upload_ms": round(float(np.median(cu)), 2),
                             "rebuilt_over_refit_pose_and_rows": round(rp / fp, 4), "rebuilt_over_refit_rows": round(rr / fr, 4),
                             "rebuilt_over_fresh_rows": round(rr / fresh, 4), "refit_over_fresh_rows": round(fr / fresh, 4)})
    if args.bench:                                                      # (3)
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
