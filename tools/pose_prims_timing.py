#!/usr/bin/env python3
"""Times a pose that states every field of a primitive (rtx_scene_pose_prims_device: the overlay kernel ahead of the pose or
rebuild kernels) beside the plain poses (rtx_scene_pose_device, rtx_scene_pose_rebuilt_device), the kernels alone.

  (a) interleaved, per scene — big_bunny + ground + 64 spheres; the 1M-triangle soup + ground; (..._1M_spheres) the same
      soup with 64 spheres, so that the overlay's primitive half runs at that size too:
      plain_refit / plain_rebuilt        rtx_scene_pose_device / rtx_scene_pose_rebuilt_device
      colours_refit / colours_rebuilt    rtx_scene_pose_prims_device with the colours given: the overlay's shading half
      all_refit / all_rebuilt            ... with spheres and colours given: the whole overlay (a scene without spheres: absent)
      overlay_*_ms in "scenes" is a DIFFERENCE of medians (prims pose - plain pose): one call's kernels share one event pair
  (b) --parent DIR    plain_refit and plain_rebuilt on the build under DIR (the parent commit's tree, built) and on this
                      one, alternated --rounds times, each a child process of this script (--root, --plain-only)
  (c) --bench         with --parent: bench.py --gpus 1 --steps 20 --warmup 3 of both builds, alternated --rounds times

Device time between two events on the launch's stream; --repeats interleaved rounds after --warmup rounds; reported are
the minimum, the median and the spread (max - min) / min.  One JSON document on stdout, and in --out.

    python tools/pose_prims_timing.py --parent ../parent --bench --out profiles/pose_prims_timing.json
"""
import argparse
import importlib
import json
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_SPHERES = 64


def summary(v):
    return {"min_ms": round(min(v), 4), "median_ms": round(float(np.median(v)), 4), "spread": round((max(v) - min(v)) / min(v), 4)}


def child(argv, cwd=None):
    r = subprocess.run([sys.executable] + argv, capture_output=True, text=True, cwd=cwd, timeout=900)
    if r.returncode != 0:
        raise SystemExit("child %s failed (%d):\n%s" % (argv, r.returncode, (r.stdout + r.stderr)[-3000:]))
    return json.loads(r.stdout[r.stdout.index("{"):]) if argv[0].endswith("pose_prims_timing.py") else \
        json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])


def spheres_in(tris, rng):
    """N_SPHERES spheres inside the mesh's box (the last triangle is the ground)"""
    pts = tris[:-1].reshape(-1, 3)
    lo, hi = pts.min(axis=0), pts.max(axis=0)
    return np.concatenate([rng.uniform(lo, hi, (N_SPHERES, 3)), rng.uniform(1.0, 6.0, (N_SPHERES, 1))], axis=1).astype(np.float32)


def measure(args, root):
    import torch  # before librtx.so: one HIP runtime per process (tests/conftest.py)
    sys.path.insert(0, root)
    rtx = importlib.import_module("ray-tracer-rust_amd")
    if rtx.device_count() < 1 or not torch.cuda.is_available():
        raise SystemExit("no HIP device: posing has no CPU fallback")
    samples = rtx.gen_samples()
    stream = torch.cuda.Stream(device="cuda:0")
    doc = {"root": os.path.relpath(root, HERE), "device": torch.cuda.get_device_name(0), "repeats": args.repeats, "warmup": args.warmup,
           "cases": [], "scenes": []}
    rng = np.random.default_rng(20)
    never = dict(reference_tree=rtx.REFTREE_NEVER, tie_rank=None)
    bunny = rtx.default_primitives([os.path.join(root, "models", "big_bunny.obj")])
    sets = [("", bunny, True, {})]
    if not args.no_1m:
        soup = rtx.synthetic_primitives(1000000)
        sets.append(("_1M", soup, False, never))
        if not args.plain_only:
            sets.append(("_1M_spheres", soup, True, never))
    with torch.cuda.stream(stream):
        s = stream.cuda_stream

        def timed(launch):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            launch()
            e1.record(stream)
            e1.synchronize()
            return e0.elapsed_time(e1)

        for tag, (t, c), with_spheres, kw in sets:
            spheres = spheres_in(t, rng) if with_spheres else None
            scene = rtx.Scene(64, 64, t, c, samples, spheres=spheres, **kw)
            scene.upload(0)
            up = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).to("cuda:0")
            d_v, d_rgb = up(t), up(rng.uniform(0.0, 1.0, c.shape))
            calls = [("plain_refit", lambda: scene.pose_device(0, d_v.data_ptr(), None, s)),
                     ("plain_rebuilt", lambda: scene.pose_rebuilt_device(0, d_v.data_ptr(), None, s))]
            if not args.plain_only:
                prims = lambda **k: (lambda: scene.pose_prims_device(0, d_v.data_ptr(), stream=s, **k))
                colours = dict(d_rgb_ptr=d_rgb.data_ptr())
                if with_spheres:
                    moved = spheres.copy()
                    moved[:, :3] += rng.uniform(-3.0, 3.0, (N_SPHERES, 3)).astype(np.float32)
                    d_s, d_srgb = up(moved), up(rng.uniform(0.0, 1.0, (N_SPHERES, 3)))
                    colours["d_sphere_rgb_ptr"] = d_srgb.data_ptr()
                    everything = dict(colours, d_spheres_ptr=d_s.data_ptr())
                    calls += [("all_refit", prims(**everything)), ("all_rebuilt", prims(rebuilt=True, **everything))]
                calls += [("colours_refit", prims(**colours)), ("colours_rebuilt", prims(rebuilt=True, **colours))]
            stream.synchronize()
            ms = {name: [] for name, _ in calls}
            for i in range(args.warmup + args.repeats):
                for name, call in calls:
                    v = timed(call)
                    if i >= args.warmup:
                        ms[name].append(v)
            row = {"scene": ("1M-triangle soup + ground" if tag else "big_bunny + ground") + (" + %d spheres" % N_SPHERES if with_spheres else ""),
                   "records": scene.info()["n_tris"], "spheres": N_SPHERES if with_spheres else 0}
            for name, v in ms.items():
                doc["cases"].append(dict(summary(v), case=name + tag))
                row[name + "_ms"] = round(float(np.median(v)), 4)
                print("%-28s min %9.4f ms  median %9.4f ms  spread %.3f" % (name + tag, min(v), float(np.median(v)), (max(v) - min(v)) / min(v)),
                      file=sys.stderr)
            for kind in ("colours", "all"):
                for tree in ("refit", "rebuilt"):
                    if "%s_%s_ms" % (kind, tree) in row:
                        row["overlay_%s_%s_ms" % (kind, tree)] = round(row["%s_%s_ms" % (kind, tree)] - row["plain_%s_ms" % tree], 4)
            doc["scenes"].append(row)
            scene.close()
            del d_v, d_rgb
    return doc


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--no-1m", action="store_true")
    ap.add_argument("--root", default=HERE, help="the tree whose build is measured (default: this one)")
    ap.add_argument("--plain-only", action="store_true", help="the plain poses only: what a parent build can run")
    ap.add_argument("--parent", default=None, help="(b), (c): the parent commit's tree, built")
    ap.add_argument("--bench", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    doc = measure(args, os.path.abspath(args.root))
    if args.parent:
        me = os.path.abspath(__file__)
        roots = (("parent", os.path.abspath(args.parent)), ("this", HERE))
        plain = {"parent": [], "this": []}
        more = ["--plain-only", "--repeats", str(args.repeats), "--warmup", str(args.warmup)] + (["--no-1m"] if args.no_1m else [])
        for k in range(args.rounds):                                      # (b); who goes first alternates too
            for who, root in roots[::-1] if k % 2 else roots:
                got = child([me, "--root", root] + more)
                plain[who].append({r["case"]: r["median_ms"] for r in got["cases"]})
        doc["plain_poses"] = {"what": "medians per child process, parent and this build alternated", **plain}
        if args.bench:                                                    # (c)
            lines = {"parent": [], "this": []}
            for k in range(args.rounds):
                for who, root in roots[::-1] if k % 2 else roots:
                    line = child([os.path.join(root, "bench.py"), "--gpus", "1", "--steps", "20", "--warmup", "3"], cwd=root)
                    lines[who].append({k: v for k, v in line.items() if not isinstance(v, (dict, list))})      # (the scalars)
            doc["bench"] = {"command": "bench.py --gpus 1 --steps 20 --warmup 3", **lines}
    text = json.dumps(doc, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
