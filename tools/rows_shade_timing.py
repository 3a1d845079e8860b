#!/usr/bin/env python3
"""Times the render pipeline's record output (rtx_render_view_rows_shade_device) on big_bunny + ground in a 1920 x 1080
frame beside its byte twin.  Kernel times are HIP events around --batch back-to-back launches on one stream, divided by the
batch.

  (1) the record launch beside the byte launch: rtx_render_view_rows_shade_device and rtx_render_view_rows*_device of this
      build (the byte launch's kernels have the parent's ISA: profiles/rows_shade_same_isa.txt), the same view and light,
      the two calls alternated, under the scene's own light and under another one; alongside, in the same rounds, a
      device-to-device hipMemcpyAsync of the 13 bytes per pixel a record has more than its three bytes, and
      rtx_render_view_device into records (the view kernel: what wrote a frame's records before).  Every compared frame is
      equal: the records' bytes to the byte launch's, the records to the view kernel's, word for word — asserted.
  (2) rtx_render_view_rows_mean_device beside rtx_render_view_mean_device — the parent's way to the same mean — at 1, 4, 16 and
      64 frames, the two alternated, the host's clock around each call with the stream waited for; every resolved frame and
      every accumulator compared word for word.  The per-frame overhead over a bare lit-rows launch: the rows mean's time per
      frame at 16 frames minus rtx_render_view_rows_lit_device's under the scene's own light given as a light.
  (3) --parent DIR [--parent2 DIR] --bench: bench.py --gpus 1 --steps 20 --warmup 3 of the builds under DIR (the parent
      commit's tree, built; a second copy of it shows the spread of two identical builds) and of this one, rotated --rounds
      times (bench.py does not reach the new code).

--repeats interleaved rounds after --warmup rounds; reported are the minimum, the median and the spread (max - min) / min.
One JSON document on stdout, and in --out.

    python tools/rows_shade_timing.py --parent ../parent --parent2 ../parent2 --bench --out profiles/rows_shade_timing.json
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
W, H = 1920, 1080
FRAME_COUNTS = (1, 4, 16, 64)
OTHER_LIGHT = ((-260.0, 280.0, 30.0, -240.0, 280.0, 30.0, -250.0, 280.0, 50.0), 100)


def summary(v):
    return {"min_ms": round(min(v), 5), "median_ms": round(float(np.median(v)), 5), "spread": round((max(v) - min(v)) / min(v), 4)}


def bench_line(root):
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--steps", "20", "--warmup", "3"],
                       capture_output=True, text=True, cwd=root, timeout=900)
    if r.returncode != 0:
        raise SystemExit("bench.py under %s failed (%d):\n%s" % (root, r.returncode, (r.stdout + r.stderr)[-3000:]))
    line = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    return {k: line[k] for k in ("value", "unit", "ms_per_step", "rays_per_frame", "primary_hits")}


def same_records(got, want):
    gl, wl = got["linear"].view(np.uint32), want["linear"].view(np.uint32)
    nan = np.isnan(want["linear"])
    return bool(np.array_equal(np.isnan(got["linear"]), nan) and np.array_equal(gl[~nan], wl[~nan])
                and np.array_equal(got["rgb8"], want["rgb8"]) and np.array_equal(got["hits"], want["hits"]))


def record_cases(args, doc):
    import torch  # before librtx.so: one HIP runtime per process (tests/conftest.py)
    sys.path.insert(0, HERE)
    rtx = importlib.import_module("ray-tracer-rust_amd")
    if rtx.device_count() < 1 or not torch.cuda.is_available():
        raise SystemExit("no HIP device: rendering has no CPU fallback")
    doc["device"] = torch.cuda.get_device_name(0)
    tris, rgb = rtx.default_primitives([os.path.join(HERE, "models", "big_bunny.obj")])
    scene = rtx.Scene(W, H, tris, rgb, rtx.gen_samples())
    scene.upload(0)
    view, n = scene.own_view(), W * H
    stream = torch.cuda.Stream(device="cuda:0")
    s = stream.cuda_stream
    d_rec, d_view, d_rgb = (torch.empty(b * n, dtype=torch.uint8, device="cuda:0") for b in (16, 16, 3))
    src, dst = (torch.empty(13 * n // 2, dtype=torch.uint8, device="cuda:0") for _ in range(2))      # a copy of B bytes moves 2 B
    lights = {"own_light": None, "other_light": rtx.Scene.make_light(*OTHER_LIGHT)}

    def events(call):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(stream):
            e0.record(stream)
            for _ in range(args.batch):
                call()
            e1.record(stream)
        stream.synchronize()
        return e0.elapsed_time(e1) / args.batch

    ms, doc["frames_equal"] = {}, {}
    for lname, light in lights.items():
        calls = {
            "rows_bytes": lambda: scene.render_view_rows_device(0, view, d_rgb.data_ptr(), 3 * n, s, light=light),
            "rows_records": lambda: scene.render_view_rows_shade_device(0, view, d_rec.data_ptr(), 16 * n, s, light=light),
            "copy_of_13_bytes_per_pixel": lambda: dst.copy_(src, non_blocking=True),
            "view_records": lambda: scene.render_view_device(0, view, d_shade_ptr=d_view.data_ptr(), stream=s, light=light),
        }
        for i in range(args.warmup + args.repeats):
            for name in list(calls)[::-1] if i % 2 else list(calls):
                with torch.cuda.stream(stream):
                    t = events(calls[name])
                if i >= args.warmup:
                    ms.setdefault("%s_%s_ms" % (name, lname), []).append(t)
        rec = d_rec.cpu().numpy().view(rtx.PIXEL_SHADE_DTYPE).reshape(H, W)
        doc["frames_equal"][lname] = {
            "records_bytes_equal_the_byte_launchs": bool(np.array_equal(rec["rgb8"], d_rgb.cpu().numpy().reshape(H, W, 3))),
            "records_equal_the_view_kernels": same_records(rec, d_view.cpu().numpy().view(rtx.PIXEL_SHADE_DTYPE).reshape(H, W)),
            "pixels_with_a_hit": int((rec["hits"] != 0).sum())}
        assert all(v for v in doc["frames_equal"][lname].values()), doc["frames_equal"][lname]
    # ---- (2) the mean of N frames: through the pipeline beside the view kernels
    n_pairs = scene.n_samples()
    d_acc, d_acc2, d_out, d_out2 = (torch.empty(16 * n, dtype=torch.uint8, device="cuda:0") for _ in range(4))
    doc["mean_frames_equal"] = {}

    def wall(call):
        stream.synchronize()
        t0 = time.perf_counter()
        call()
        stream.synchronize()
        return 1e3 * (time.perf_counter() - t0)

    for count in FRAME_COUNTS:
        seeds = [1000 + k for k in range(count)]
        repeats = max(2, args.repeats // (1 if count <= 4 else 2 if count == 16 else 4))
        ways = {
            "rows_mean_device_%d_frames_ms" % count: lambda: scene.render_view_mean_device(
                0, view, seeds, n_pairs, d_acc.data_ptr(), None, d_out.data_ptr(), s, rows=True),
            "view_mean_device_%d_frames_ms" % count: lambda: scene.render_view_mean_device(
                0, view, seeds, n_pairs, d_acc2.data_ptr(), None, d_out2.data_ptr(), s),
        }
        for i in range(1 + repeats):
            for name in list(ways)[::-1] if i % 2 else list(ways):
                t = wall(ways[name])
                if i >= 1:
                    ms.setdefault(name, []).append(t)
        rec, rec2 = (d.cpu().numpy().view(rtx.PIXEL_SHADE_DTYPE).reshape(H, W) for d in (d_out, d_out2))
        acc, acc2 = (d.cpu().numpy().view(rtx.ACCUM_PIXEL_DTYPE).reshape(H, W) for d in (d_acc, d_acc2))
        nan = np.isnan(acc2["sum"])
        doc["mean_frames_equal"][str(count)] = {
            "records_equal": same_records(rec, rec2),
            "accumulators_equal": bool(np.array_equal(np.isnan(acc["sum"]), nan) and np.array_equal(acc["sum"].view(np.uint32)[~nan], acc2["sum"].view(np.uint32)[~nan])
                                       and np.array_equal(acc["hit_frames"], acc2["hit_frames"]))}
        assert all(doc["mean_frames_equal"][str(count)].values()), (count, doc["mean_frames_equal"][str(count)])
    own_given = scene.light()
    for i in range(args.warmup + args.repeats):
        t = events(lambda: scene.render_view_rows_device(0, view, d_rgb.data_ptr(), 3 * n, s, light=own_given))
        if i >= args.warmup:
            ms.setdefault("rows_lit_bare_own_light_given_ms", []).append(t)
    scene.close()
    doc["cases"] = [dict(case=k, **summary(v)) for k, v in ms.items()]
    med = {k: float(np.median(v)) for k, v in ms.items()}
    doc["differences_of_medians"] = {}
    for lname in lights:
        b, r, c = (med["%s_%s_ms" % (k, lname)] for k in ("rows_bytes", "rows_records", "copy_of_13_bytes_per_pixel"))
        spread = (max(ms["rows_bytes_%s_ms" % lname]) - min(ms["rows_bytes_%s_ms" % lname]))
        doc["differences_of_medians"][lname] = {
            "records_minus_bytes_ms": round(r - b, 5), "records_over_bytes": round(r / b, 4), "copy_ms": round(c, 5),
            "spread_of_the_byte_launch_ms": round(spread, 5),
            "records_slower_by_more_than_copy_plus_spread": bool(r - b > c + spread),
            "view_kernel_over_records": round(med["view_records_%s_ms" % lname] / r, 2)}
    doc["mean"] = {}
    for count in FRAME_COUNTS:
        r, v = med["rows_mean_device_%d_frames_ms" % count], med["view_mean_device_%d_frames_ms" % count]
        doc["mean"][str(count)] = {"rows_mean_ms": round(r, 4), "view_mean_ms": round(v, 4), "view_over_rows": round(v / r, 2),
                                   "rows_mean_per_frame_ms": round(r / count, 4), "view_mean_per_frame_ms": round(v / count, 4)}
    doc["mean"]["per_frame_overhead_over_a_bare_lit_rows_launch_ms"] = round(
        med["rows_mean_device_16_frames_ms"] / 16 - med["rows_lit_bare_own_light_given_ms"], 4)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--parent")
    ap.add_argument("--parent2")
    ap.add_argument("--bench", action="store_true")
    ap.add_argument("--out")
    args = ap.parse_args()
    doc = {"frame": [W, H], "scene": "big_bunny.obj + ground, the scene's own view", "repeats": args.repeats, "batch": args.batch}
    record_cases(args, doc)
    if args.parent and args.bench:                                        # (2); the order rotates
        roots = [("parent", os.path.abspath(args.parent)), ("this", HERE)]
        if args.parent2:
            roots.append(("parent2", os.path.abspath(args.parent2)))
        lines = {who: [] for who, _ in roots}
        for k in range(args.rounds):
            for who, root in roots[k % len(roots):] + roots[:k % len(roots)]:
                lines[who].append(bench_line(root))
        doc["bench"] = {"command": "bench.py --gpus 1 --steps 20 --warmup 3", **lines}
    text = json.dumps(doc, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
