#!/usr/bin/env python3
"""Times a new sample table per frame on a scene that stays uploaded (rtx_scene_resample, rtx_scene_reseed: the host calls,
each device's catch-up, the sample-table kernel) beside what the parent commit can do for a new table — a new scene — on
big_bunny + ground in a 1920 x 1080 frame.  All wall times are the host's clock around the calls, the stream waited for.

  (1) host calls: rtx_scene_resample with 2,000,000 pairs, rtx_scene_reseed at 2,000 and at 2,000,000 pairs (no work
      proportional to the pair count shows here).
  (2) one device's catch-up, rtx_scene_upload right behind a replacement on an idle device: behind a reseed and behind a
      resample, each at 2 pairs (the fixed part: the device wait, the launch or copy call, the small light uploads) and at
      2,000,000 pairs.  `device_wait` is a device synchronisation of the idle device alone.
  (3) the kernel beside a copy of the same table: the 2,000,000-pair catch-up minus the 2-pair one, of the reseed (the
      kernel) and of the resample (the library's 16 MB hipMemcpy from pageable memory) — DIFFERENCES of medians, since the
      catch-up is one synchronous call — and a 16 MB torch host-to-device copy from pageable memory between the same clocks.
  (4) per frame, four tables, interleaved: `reseed` — rtx_scene_reseed + rtx_render_view_rows_device of the scene's own
      view; `resample` — rtx_scene_resample of the same table made by the caller beforehand + the same launch; `fresh` — the
      yardstick: rtx_scene_create with the table + rtx_scene_upload + the same launch + destroy.  Every frame of the first two
      is compared byte for byte with the fresh scene's.  Each replacement runs behind one of its own kind — a table per
      frame — and is also timed in its parts (host call, catch-up through rtx_scene_upload, the frame); `first_*` is the
      same behind a table of the OTHER kind, where the scene's 16 MB host array is given back or allocated; `rows_alone`
      and `rows_behind_the_fresh_scene` are the frame with nothing replaced.
  (5) --parent DIR [--parent2 DIR] --bench: bench.py --gpus 1 --steps 20 --warmup 3 of the builds under DIR (the parent
      commit's tree, built; a second copy of it shows the spread of two identical builds) and of this one, alternated
      --rounds times (bench.py does not reach the new code).

--repeats interleaved rounds after --warmup rounds; reported are the minimum, the median and the spread (max - min) / min.
One JSON document on stdout, and in --out.

    python tools/resample_timing.py --parent ../parent --parent2 ../parent2 --bench --out profiles/resample_timing.json
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
PAIRS = 2000000
FRAME_SEEDS = (101, 102, 103, 104)


def summary(v):
    return {"min_ms": round(min(v), 4), "median_ms": round(float(np.median(v)), 4), "spread": round((max(v) - min(v)) / min(v), 4)}


def bench_line(root):
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--steps", "20", "--warmup", "3"],
                       capture_output=True, text=True, cwd=root, timeout=900)
    if r.returncode != 0:
        raise SystemExit("bench.py under %s failed (%d):\n%s" % (root, r.returncode, (r.stdout + r.stderr)[-3000:]))
    line = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    return {k: v for k, v in line.items() if not isinstance(v, (dict, list))}      # (the scalars)


def measure(args):
    import torch  # before librtx.so: one HIP runtime per process (tests/conftest.py)
    sys.path.insert(0, HERE)
    rtx = importlib.import_module("ray-tracer-rust_amd")
    if rtx.device_count() < 1 or not torch.cuda.is_available():
        raise SystemExit("no HIP device: rendering has no CPU fallback")
    W, H = 1920, 1080
    tris, rgb = rtx.default_primitives([os.path.join(HERE, "models", "big_bunny.obj")])
    created = rtx.gen_samples()
    stream = torch.cuda.Stream(device="cuda:0")
    s = stream.cuda_stream
    doc = {"device": torch.cuda.get_device_name(0), "repeats": args.repeats, "warmup": args.warmup, "frame": [W, H],
           "pairs": PAIRS, "table_bytes": 8 * PAIRS, "cases": [], "frames": []}
    ms = {}

    def add(name, v):
        ms.setdefault(name, []).append(v)

    def wall(call):
        t0 = time.perf_counter()
        call()
        return 1e3 * (time.perf_counter() - t0)

    scene = rtx.Scene(W, H, tris, rgb, created)
    scene.upload(0)
    view = scene.own_view()
    nbytes = H * W * 3
    buf = torch.empty(nbytes, dtype=torch.uint8, device="cuda:0")
    big = [rtx.gen_samples(1 + k, PAIRS) for k in range(2)]
    small = [rtx.gen_samples(1 + k, 2) for k in range(2)]
    host_table = torch.from_numpy(big[0].copy())
    dev_table = torch.empty_like(host_table, device="cuda:0")
    rounds = args.warmup + args.repeats
    # (1), (2), (3)
    for i in range(rounds):
        keep = i >= args.warmup
        row = {}
        row["host_resample_2M_ms"] = wall(lambda: scene.resample(big[i % 2]))
        row["catch_up_resample_2M_ms"] = wall(lambda: scene.upload(0))
        row["host_reseed_2k_ms"] = wall(lambda: scene.reseed(50 + i, 2000))
        scene.upload(0)
        row["host_reseed_2M_ms"] = wall(lambda: scene.reseed(70 + i, PAIRS))
        row["catch_up_reseed_2M_ms"] = wall(lambda: scene.upload(0))
        scene.reseed(90 + i, 2)
        row["catch_up_reseed_2_ms"] = wall(lambda: scene.upload(0))
        scene.resample(small[i % 2])
        row["catch_up_resample_2_ms"] = wall(lambda: scene.upload(0))
        row["device_wait_idle_ms"] = wall(torch.cuda.synchronize)
        row["upload_with_nothing_to_do_ms"] = wall(lambda: scene.upload(0))

        def copy():
            dev_table.copy_(host_table)
            torch.cuda.synchronize()
        row["torch_copy_16MB_pageable_ms"] = wall(copy)
        if keep:
            for k, v in row.items():
                add(k, v)
    # (4)
    tables = {seed: rtx.gen_samples(seed, PAIRS) for seed in FRAME_SEEDS}
    want = {}
    for i in range(rounds):
        keep = i >= args.warmup
        for seed in FRAME_SEEDS:
            def fresh():
                with rtx.Scene(W, H, tris, rgb, tables[seed]) as f:
                    f.upload(0)
                    f.render_view_rows_device(0, f.own_view(), buf.data_ptr(), nbytes, s)
                    stream.synchronize()
            t_fresh = wall(fresh)
            if seed not in want:
                want[seed] = buf.cpu().numpy().copy()

            def rows_alone():
                scene.render_view_rows_device(0, view, buf.data_ptr(), nbytes, s)
                stream.synchronize()
            t_rows_before = wall(rows_alone)                        # the standing scene's frame right behind the fresh one's

            # each kind of replacement twice: behind a table of the other kind (`first`: the scene's host array is given back
            # or allocated) and behind one of its own kind (what a table per frame costs), the latter compared and once more
            # in its parts: the host call, the catch-up, the frame
            other = tables[FRAME_SEEDS[(FRAME_SEEDS.index(seed) + 1) % len(FRAME_SEEDS)]]

            def replaced(call):
                call()
                rows_alone()
            t_reseed_first = wall(lambda: replaced(lambda: scene.reseed(seed + 1000, PAIRS)))
            t_reseed = wall(lambda: replaced(lambda: scene.reseed(seed, PAIRS)))
            bad_reseed = int((buf.cpu().numpy() != want[seed]).sum())
            parts_reseed = [wall(lambda: scene.reseed(seed + 2000, PAIRS)), wall(lambda: scene.upload(0)), wall(rows_alone)]
            t_resample_first = wall(lambda: replaced(lambda: scene.resample(other)))
            t_resample = wall(lambda: replaced(lambda: scene.resample(tables[seed])))
            bad_resample = int((buf.cpu().numpy() != want[seed]).sum())
            parts_resample = [wall(lambda: scene.resample(other)), wall(lambda: scene.upload(0)), wall(rows_alone)]
            t_rows = wall(rows_alone)
            if keep:
                add("frame_fresh_scene_ms", t_fresh)
                add("frame_reseed_plus_rows_ms", t_reseed)
                add("frame_resample_plus_rows_ms", t_resample)
                add("frame_first_reseed_behind_a_resample_plus_rows_ms", t_reseed_first)
                add("frame_first_resample_behind_a_reseed_plus_rows_ms", t_resample_first)
                add("frame_rows_alone_ms", t_rows)
                add("frame_rows_behind_the_fresh_scene_ms", t_rows_before)
                for what, parts in (("reseed", parts_reseed), ("resample", parts_resample)):
                    for part, v in zip(("host_call", "catch_up", "rows"), parts):
                        add("frame_%s_part_%s_ms" % (what, part), v)
            if i == rounds - 1:
                doc["frames"].append({"seed": seed, "fresh_scene_ms": round(t_fresh, 4), "reseed_plus_rows_ms": round(t_reseed, 4),
                                      "resample_plus_rows_ms": round(t_resample, 4), "differing_bytes_reseed": bad_reseed,
                                      "differing_bytes_resample": bad_resample})
            if bad_reseed or bad_resample:
                raise SystemExit("seed %d: %d / %d bytes differ from the fresh scene's frame" % (seed, bad_reseed, bad_resample))
    scene.close()
    med = {}
    for name, v in ms.items():
        doc["cases"].append(dict(summary(v), case=name[:-3]))
        med[name] = float(np.median(v))
        print("%-34s min %9.4f ms  median %9.4f ms  spread %.3f" % (name[:-3], min(v), med[name], (max(v) - min(v)) / min(v)), file=sys.stderr)
    doc["differences_of_medians"] = {
        "kernel_2M_ms": round(med["catch_up_reseed_2M_ms"] - med["catch_up_reseed_2_ms"], 4),
        "library_copy_2M_ms": round(med["catch_up_resample_2M_ms"] - med["catch_up_resample_2_ms"], 4),
        "small_uploads_and_launch_ms": round(med["catch_up_reseed_2_ms"] - med["upload_with_nothing_to_do_ms"], 4)}
    return doc


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--parent", default=None, help="(5): the parent commit's tree, built")
    ap.add_argument("--parent2", default=None, help="(5): a second copy of it")
    ap.add_argument("--bench", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    doc = measure(args)
    if args.parent and args.bench:                                        # (5); who goes first alternates too
        roots = [("parent", os.path.abspath(args.parent)), ("this", HERE)]
        if args.parent2:
            roots.append(("parent2", os.path.abspath(args.parent2)))
        lines = {who: [] for who, _ in roots}
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
