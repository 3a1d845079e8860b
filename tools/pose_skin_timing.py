#!/usr/bin/env python3
"""Times a skinned pose (rtx_scene_pose_skinned / _device: the skin kernel ahead of the overlay and pose or rebuild kernels)
beside the poses that are handed vertices and beside a moved pose, on big_bunny + ground and on the 1M-triangle soup +
ground, both in a 1920 x 1080 frame.  The motion is a bend: the mesh's foot stays, its head turns about the vertical through
the mesh's box centre, and every corner blends the two by its height; the ground's bones are all RTX_MOVE_NONE.

  (a) host calls, interleaved: `numpy` — the bend of every vertex in numpy float32 (two maps and a blend), what a caller of
      rtx_scene_pose does per frame — and `pose` — rtx_scene_pose on those vertices; beside them `skinned` —
      rtx_scene_pose_skinned for the same bend.  Each call as the host's wall time around it (*_wall_ms) and as its
      RtxStats.total_ms / kernel_ms.  The wall time of `skinned` includes the range rule over the host statement, which runs
      before RtxStats' clock starts.
  (b) device calls between two events on the launch's stream, interleaved: rtx_scene_pose_device on resident vertices and
      rtx_scene_pose_moved_device (one turn; the parent commit's kernels, the yardstick) beside
      rtx_scene_pose_skinned_device under a skin of one weighted bone per corner (`one`) and of four (`four`), refitted and
      rebuilt.  The skin is bound and one untimed pose uploads it before each timed call of the round.  skin_*_ms in
      "scenes" is a DIFFERENCE of medians against the moved pose: one call's kernels share one event pair.
  (c) four frames of the bend as rtx_scene_pose_skinned_device + rtx_render_view_rows_posed_device on one stream, between
      events; every frame compared byte for byte with the frame over rtx_scene_pose of rtx_scene_skinned_prims' vertices.
  (d) --parent DIR --bench: bench.py --gpus 1 --steps 20 --warmup 3 of the build under DIR (the parent commit's tree, built)
      and of this one, alternated --rounds times (bench.py does not reach the new code).

--repeats interleaved rounds after --warmup rounds; reported are the minimum, the median and the spread (max - min) / min.
One JSON document on stdout, and in --out.

    python tools/pose_skin_timing.py --parent ../parent --bench --out profiles/pose_skin_timing.json
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
F = np.float32
IDENTITY = np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], F)


def summary(v):
    return {"min_ms": round(min(v), 4), "median_ms": round(float(np.median(v)), 4), "spread": round((max(v) - min(v)) / min(v), 4)}


def bench_line(root):
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--steps", "20", "--warmup", "3"],
                       capture_output=True, text=True, cwd=root, timeout=900)
    if r.returncode != 0:
        raise SystemExit("bench.py under %s failed (%d):\n%s" % (root, r.returncode, (r.stdout + r.stderr)[-3000:]))
    line = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    return {k: v for k, v in line.items() if not isinstance(v, (dict, list))}      # (the scalars)


def turn_of(tris, degrees):
    """the move (12 floats, composed in double, rounded once) that turns the mesh — every triangle but the last, the
    ground — about the vertical through its box centre"""
    pts = tris[:-1].reshape(-1, 3).astype(np.float64)
    c = 0.5 * (pts.min(axis=0) + pts.max(axis=0))
    a = np.deg2rad(degrees)
    lin = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
    return np.concatenate([lin, (c - lin @ c).reshape(3, 1)], axis=1).reshape(12).astype(F)


def heights(tris):
    """per corner of the mesh [n - 1, 3]: 0 at its lowest vertex, 1 at its highest"""
    y = tris[:-1].reshape(-1, 3, 3)[:, :, 1]
    return ((y - y.min()) / (y.max() - y.min())).astype(F)


def skins(tris):
    """name -> keywords of rtx.Scene.skin: `bend` (two bones, weights by height), `one` (one bone of weight 1), `four`
    (four bones, fixed weights); the ground — the last triangle — all RTX_MOVE_NONE"""
    n = len(tris)
    none = 0xFFFFFFFF
    out = {}
    for name in ("bend", "one", "four"):
        bones = np.full((n, 3, 4), none, np.uint32)
        weights = np.zeros((n, 3, 4), F)
        if name == "bend":
            h = heights(tris)
            bones[:-1, :, 0], bones[:-1, :, 1] = 0, 1
            weights[:-1, :, 0], weights[:-1, :, 1] = 1.0 - h, h
        elif name == "one":
            bones[:-1, :, 0] = 0
            weights[:-1, :, 0] = 1.0
        else:
            bones[:-1] = np.arange(4, dtype=np.uint32)
            weights[:-1] = np.array([0.4, 0.3, 0.2, 0.1], F)
        out[name] = dict(bones=bones, weights=weights)
    return out


def bent_in_numpy(tris, moves, h):
    """what a caller of rtx_scene_pose computes per frame: every mesh vertex through both maps and the blend, float32, the
    ground as it is"""
    out = np.empty_like(tris)
    p = tris[:-1].reshape(-1, 3)
    q = [(p @ m.reshape(3, 4)[:, :3].T + m.reshape(3, 4)[:, 3]) for m in moves]
    w = h.reshape(-1, 1)
    out[:-1] = ((1.0 - w) * q[0] + w * q[1]).astype(F).reshape(-1, 9)
    out[-1] = tris[-1]
    return out


def measure(args):
    import torch  # before librtx.so: one HIP runtime per process (tests/conftest.py)
    sys.path.insert(0, HERE)
    rtx = importlib.import_module("ray-tracer-rust_amd")
    if rtx.device_count() < 1 or not torch.cuda.is_available():
        raise SystemExit("no HIP device: posing has no CPU fallback")
    samples = rtx.gen_samples()
    stream = torch.cuda.Stream(device="cuda:0")
    doc = {"device": torch.cuda.get_device_name(0), "repeats": args.repeats, "warmup": args.warmup, "frame": [1920, 1080],
           "cases": [], "scenes": [], "frames": []}
    never = dict(reference_tree=rtx.REFTREE_NEVER, tie_rank=None)
    sets = [("", "big_bunny + ground", rtx.default_primitives([os.path.join(HERE, "models", "big_bunny.obj")]), {})]
    if not args.no_1m:
        sets.append(("_1M", "1M-triangle soup + ground", rtx.synthetic_primitives(1000000), never))
    with torch.cuda.stream(stream):
        s = stream.cuda_stream

        def timed(launch):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            launch()
            e1.record(stream)
            e1.synchronize()
            return e0.elapsed_time(e1)

        for tag, title, (t, c), kw in sets:
            t = np.ascontiguousarray(t, F)
            scene = rtx.Scene(1920, 1080, t, c, samples, **kw)
            scene.upload(0)
            n = len(t)
            group = np.zeros(n, np.uint32)
            group[-1] = rtx.rtx.MOVE_NONE                               # the ground
            h = heights(t)
            skin = skins(t)
            bend = np.stack([IDENTITY, turn_of(t, 40.0)])
            four = np.stack([turn_of(t, d) for d in (10.0, 20.0, 30.0, 40.0)])
            ms = {}

            def add(name, v):
                ms.setdefault(name, []).append(v)

            # (a) host calls
            scene.skin(**skin["bend"])
            for i in range(args.warmup + args.repeats):
                t0 = time.perf_counter()
                v = bent_in_numpy(t, bend, h)
                t1 = time.perf_counter()
                st = scene.pose(v, stats=True)
                t2 = time.perf_counter()
                sm = scene.pose_skinned(bend, stats=True)
                t3 = time.perf_counter()
                if i >= args.warmup:
                    add("host_numpy_wall_ms", 1e3 * (t1 - t0))
                    add("host_pose_wall_ms", 1e3 * (t2 - t1))
                    add("host_pose_total_ms", st["total_ms"])
                    add("host_pose_kernel_ms", st["kernel_ms"])
                    add("host_skinned_wall_ms", 1e3 * (t3 - t2))
                    add("host_skinned_total_ms", sm["total_ms"])
                    add("host_skinned_kernel_ms", sm["kernel_ms"])
            # (b) device calls
            up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")
            d_v, d_g = up(bent_in_numpy(t, bend, h)), up(group.view(np.int32))
            d_turn, d_four = up(four[3:]), up(four)
            plain = [("device_pose_refit_ms", lambda: scene.pose_device(0, d_v.data_ptr(), None, s)),
                     ("device_moved_refit_ms", lambda: scene.pose_moved_device(0, 1, d_turn.data_ptr(), d_g.data_ptr(), stream=s)),
                     ("device_moved_rebuilt_ms", lambda: scene.pose_moved_device(0, 1, d_turn.data_ptr(), d_g.data_ptr(), rebuilt=True, stream=s))]
            skinned = [("one", 1, d_turn), ("four", 4, d_four)]
            stream.synchronize()
            for i in range(args.warmup + args.repeats):
                for name, call in plain:
                    v = timed(call)
                    if i >= args.warmup:
                        add(name, v)
                for which, n_moves, d_m in skinned:
                    scene.skin(**skin[which])
                    scene.pose_skinned_device(0, n_moves, d_m.data_ptr(), stream=s)          # (untimed: uploads the skin)
                    stream.synchronize()
                    for tree, rebuilt in (("refit", False), ("rebuilt", True)):
                        v = timed(lambda: scene.pose_skinned_device(0, n_moves, d_m.data_ptr(), rebuilt=rebuilt, stream=s))
                        if i >= args.warmup:
                            add("device_skinned_%s_%s_ms" % (which, tree), v)
            row = {"scene": title, "records": scene.info()["n_tris"], "pose_bytes_per_frame": 36 * n,
                   "skinned_bytes_per_frame": 96, "skin_bytes_bound_once": 96 * n}
            for name, v in ms.items():
                doc["cases"].append(dict(summary(v), case=name[:-3] + tag))
                row[name] = round(float(np.median(v)), 4)
                print("%-34s min %9.4f ms  median %9.4f ms  spread %.3f" % (name[:-3] + tag, min(v), float(np.median(v)),
                                                                            (max(v) - min(v)) / min(v)), file=sys.stderr)
            row["host_numpy_plus_pose_wall_ms"] = round(row["host_numpy_wall_ms"] + row["host_pose_wall_ms"], 4)
            for which in ("one", "four"):
                for tree in ("refit", "rebuilt"):
                    row["skin_%s_%s_over_moved_ms" % (which, tree)] = round(row["device_skinned_%s_%s_ms" % (which, tree)] -
                                                                           row["device_moved_%s_ms" % tree], 4)
            doc["scenes"].append(row)
            # (c) four frames of the bend
            scene.skin(**skin["bend"])
            view = scene.own_view()
            nbytes = 1080 * 1920 * 3
            buf = torch.empty(nbytes, dtype=torch.uint8, device="cuda:0")
            for k, degrees in enumerate((25.0, 50.0, 75.0, 100.0)):
                mk = np.stack([IDENTITY, turn_of(t, degrees)])
                d_mk = up(mk)
                stream.synchronize()

                def frame():
                    scene.pose_skinned_device(0, 2, d_mk.data_ptr(), stream=s)
                    scene.render_view_rows_device(0, view, buf.data_ptr(), nbytes, s, posed=True)
                pair = timed(frame)
                got = buf.cpu().numpy().reshape(1080, 1920, 3)
                v, _ = scene.skinned_prims(mk)
                scene.pose(v)
                want = scene.render_view_rows(view, posed=True)
                doc["frames"].append({"scene": title, "degrees": degrees, "skinned_pose_plus_rows_ms": round(pair, 4),
                                      "differing_bytes": int((got != want).sum())})
                print("bend %3.0f of %-28s %9.4f ms, %d differing bytes" % (degrees, title, pair, doc["frames"][-1]["differing_bytes"]),
                      file=sys.stderr)
            scene.close()
            del d_v, d_g, d_turn, d_four, buf
    return doc


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--no-1m", action="store_true")
    ap.add_argument("--parent", default=None, help="(d): the parent commit's tree, built")
    ap.add_argument("--bench", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    doc = measure(args)
    if args.parent and args.bench:                                        # (d); who goes first alternates too
        roots = (("parent", os.path.abspath(args.parent)), ("this", HERE))
        lines = {"parent": [], "this": []}
        for k in range(args.rounds):
            for who, root in roots[::-1] if k % 2 else roots:
                lines[who].append(bench_line(root))
        doc["bench"] = {"command": "bench.py --gpus 1 --steps 20 --warmup 3", **lines}
    text = json.dumps(doc, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
