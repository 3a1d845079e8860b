#!/usr/bin/env python3
"""Times the adaptive mean through the render pipeline (rtx_render_view_rows_adaptive_device) on big_bunny + ground in a
1920 x 1080 frame.  The yardsticks are this build's rtx_render_view_rows_mean_device and rtx_render_view_adaptive_device at the
same N, alternated with the call under test in one run.  Call times are HIP events around one whole call on a stream of its
own; kernel times are events around --batch back-to-back launches, divided by the batch.

  (1) rtx_moment_add_device and rtx_accum_add_device over the frame (their difference is what the adaptive call's add costs
      over the mean's) and a device-to-device copy of the 32 extra bytes per pixel a moment add moves.
  (2) at 16 and 64 frames, per round: the pipeline mean, the view kernel's adaptive call and the pipeline's under the rule
      that never stops (min_frames = N), under a rule that stops everything at 2 (max_variance = +infinity), and under
      --middle thresholds taken from the tile errors the never-stopping run leaves (their quantiles over the tiles whose
      error is not 0).  For each: the share of tile-frames rendered (from the tile states), the time, the ratio to both
      yardsticks.  With min_frames = N the outputs, sums and hit counts are compared word for word with the pipeline mean's,
      and under every rule moments, tile states, records and bytes with the view kernel's adaptive call.
  (3) what a frame costs in which every tile has stopped (it still runs the sample-table kernel, the light's kernels and the
      pipeline's dispatches), and the passes of the late frames of the run under the highest threshold — few, costly tiles —
      beside the pipeline mean's, from rtx_launch_timings.
  (4) --parent DIR --bench: bench.py --gpus 1 --steps 20 --warmup 3 of the build under DIR (the parent commit's tree, built)
      and of this one, alternated --rounds times (bench.py does not reach the new code).

--repeats interleaved rounds after one warm-up round; reported are the minimum, the median and the spread (max - min) / min.
One JSON document on stdout, and in --out.

    python tools/rows_adapt_timing.py --parent build_ab/parent --bench --out profiles/rows_adapt_timing.json
"""
import argparse
import importlib
import json
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = 1920, 1080
FRAME_COUNTS = (16, 64)
INF = float("inf")


def summary(v):
    return {"min_ms": round(min(v), 5), "median_ms": round(float(np.median(v)), 5), "spread": round((max(v) - min(v)) / min(v), 4)}


def bench_line(root):
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--steps", "20", "--warmup", "3"],
                       capture_output=True, text=True, cwd=root, timeout=900)
    if r.returncode != 0:
        raise SystemExit("bench.py under %s failed (%d):\n%s" % (root, r.returncode, (r.stdout + r.stderr)[-3000:]))
    line = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    return {k: v for k, v in line.items() if not isinstance(v, (dict, list))}      # (the scalars)


class Bench:
    def __init__(self, args):
        import torch  # before librtx.so: one HIP runtime per process (tests/conftest.py)
        sys.path.insert(0, HERE)
        self.torch = torch
        self.rtx = rtx = importlib.import_module("ray-tracer-rust_amd")
        if rtx.device_count() < 1 or not torch.cuda.is_available():
            raise SystemExit("no HIP device: rendering has no CPU fallback")
        self.args = args
        tris, rgb = rtx.default_primitives([os.path.join(HERE, "models", "big_bunny.obj")])
        self.scene = rtx.Scene(W, H, tris, rgb, rtx.gen_samples())
        self.scene.upload(0)
        self.view = self.scene.own_view()
        self.n = W * H
        self.tiles_x, self.tiles_y = rtx.tile_grid(W, H)
        self.n_tiles = self.tiles_x * self.tiles_y
        self.stream = torch.cuda.Stream(device="cuda:0")
        self.s = self.stream.cuda_stream
        self.ms = {}

    def dev(self, nbytes):
        return self.torch.empty(nbytes, dtype=self.torch.uint8, device="cuda:0")

    def add(self, name, v):
        self.ms.setdefault(name, []).append(v)

    def events(self, call, batch=None):
        """device time of one call, HIP events around `batch` of them on the stream"""
        batch = batch or self.args.batch
        t = self.torch
        e0, e1 = t.cuda.Event(enable_timing=True), t.cuda.Event(enable_timing=True)
        with t.cuda.stream(self.stream):
            e0.record(self.stream)
            for _ in range(batch):
                call()
            e1.record(self.stream)
        self.stream.synchronize()
        return e0.elapsed_time(e1) / batch

    def tiles_of(self, d_tiles):
        self.stream.synchronize()
        return d_tiles.cpu().numpy().view(self.rtx.TILE_STATE_DTYPE).reshape(self.tiles_y, self.tiles_x)

    # ---- (1)
    def kernel_cases(self):
        sc, n, s = self.scene, self.n, self.s
        rec, mom, acc, tiles = self.dev(16 * n), self.dev(32 * n), self.dev(16 * n), self.dev(8 * self.n_tiles)
        never = (1 << 20, 0.0)
        sc.render_view_rows_shade_device(0, self.view, rec.data_ptr(), 16 * n, s)
        sc.moment_add_device(0, W, H, rec.data_ptr(), mom.data_ptr(), tiles.data_ptr(), True, never, s)
        sc.accum_add_device(0, n, rec.data_ptr(), acc.data_ptr(), True, s)
        self.stream.synchronize()
        P = lambda t: t.data_ptr()
        src, dst = self.dev(16 * n), self.dev(16 * n)                   # a copy of B bytes moves 2 B: 32 bytes per pixel moved
        cases = {"moment_add": lambda: sc.moment_add_device(0, W, H, P(rec), P(mom), P(tiles), False, never, s),
                 "accum_add": lambda: sc.accum_add_device(0, n, P(rec), P(acc), False, s),
                 "copy_of_32_bytes_per_pixel": lambda: dst.copy_(src, non_blocking=True)}
        for i in range(1 + self.args.repeats):
            for name, call in cases.items():
                t = self.events(call)
                if i >= 1:
                    self.add("kernel_%s_ms" % name, t)

    # ---- (2), (3)
    def frames(self, doc):
        sc, rtx, n, s = self.scene, self.rtx, self.n, self.s
        n_pairs = sc.n_samples()
        acc, mom, tiles, mom_v, tiles_v = self.dev(16 * n), self.dev(32 * n), self.dev(8 * self.n_tiles), self.dev(32 * n), self.dev(8 * self.n_tiles)
        rgb, rgb2, shade, shade2 = self.dev(3 * n), self.dev(3 * n), self.dev(16 * n), self.dev(16 * n)
        P = lambda t: t.data_ptr()
        doc["frames"] = []
        for count in FRAME_COUNTS:
            seeds = [3000 + k for k in range(count)]
            mean = lambda: sc.render_view_mean_device(0, self.view, seeds, n_pairs, P(acc), P(rgb2), P(shade2), s, rows=True)
            rows = lambda rule: sc.render_view_rows_adaptive_device(0, self.view, seeds, rule, n_pairs, P(mom), P(tiles), P(rgb), P(shade), s)
            view = lambda rule: sc.render_view_adaptive_device(0, self.view, seeds, rule, n_pairs, P(mom_v), P(tiles_v), P(rgb2), P(shade2), s)
            # the never-stopping run against the pipeline mean, word for word; its tile errors give the middle thresholds
            self.events(mean, batch=1)
            self.events(lambda: rows((count, 0.0)), batch=1)
            self.stream.synchronize()
            m = mom.cpu().numpy().view(rtx.MOMENT_PIXEL_DTYPE)
            a = acc.cpu().numpy().view(rtx.ACCUM_PIXEL_DTYPE)
            same = (m["sum"].tobytes() == a["sum"].tobytes() and np.array_equal(m["hit_frames"], a["hit_frames"])
                    and bool(self.torch.equal(rgb, rgb2)) and bool(self.torch.equal(shade, shade2)))
            if not same:
                raise SystemExit("%d frames: min_frames = N differs from rtx_render_view_rows_mean_device" % count)
            err = self.tiles_of(tiles)["err"]
            quantiles = [float(q) for q in np.quantile(err[err > 0], self.args.middle)]
            rules = {"never_stops": (count, 0.0), "stops_everything_at_2": (2, INF)}
            for q, thr in zip(self.args.middle, quantiles):
                rules["middle_q%02d" % round(100 * q)] = (2, thr)
            # every rule against the view kernel's adaptive call, word for word
            for name, rule in rules.items():
                self.events(lambda: rows(rule), batch=1)
                self.events(lambda: view(rule), batch=1)
                self.stream.synchronize()
                if not all(bool(self.torch.equal(x, y)) for x, y in ((mom, mom_v), (tiles, tiles_v), (rgb, rgb2), (shade, shade2))):
                    raise SystemExit("%d frames, %s: differs from rtx_render_view_adaptive_device" % (count, name))
            order = ["rows_mean"] + ["view_" + r for r in rules] + list(rules)
            repeats = max(3, self.args.repeats // (1 if count <= 16 else 2))
            share, passes = {}, {}
            for i in range(1 + repeats):
                for name in order[::-1] if i % 2 else order:
                    if name == "rows_mean":
                        t = self.events(mean, batch=1)
                        passes[name] = sc.launch_timings()
                    elif name.startswith("view_"):
                        t = self.events(lambda: view(rules[name[5:]]), batch=1)
                    else:
                        t = self.events(lambda: rows(rules[name]), batch=1)
                        share[name] = float(self.tiles_of(tiles)["frames"].astype(np.float64).sum() / (self.n_tiles * count))
                        passes[name] = sc.launch_timings()
                    if i >= 1:
                        self.add("%s_%d_frames_ms" % (name, count), t)
            entry = {"frames": count, "equal_to_the_rows_mean_with_min_frames_n": True,
                     "equal_to_the_view_kernels_adaptive_call_under_every_rule": True, "rules": {}}
            med = {name: float(np.median(self.ms["%s_%d_frames_ms" % (name, count)])) for name in order}
            for name, rule in rules.items():
                entry["rules"][name] = {"min_frames": rule[0], "max_variance": rule[1] if rule[1] != INF else "inf",
                                        "share_of_tile_frames_rendered": round(share[name], 4), "median_ms": round(med[name], 4),
                                        "per_frame_ms": round(med[name] / count, 5),
                                        "view_kernels_adaptive_call_ms": round(med["view_" + name], 4),
                                        "over_view_adaptive": round(med[name] / med["view_" + name], 4),
                                        "over_rows_mean": round(med[name] / med["rows_mean"], 4),
                                        "beats_the_pipeline_mean": bool(med[name] < med["rows_mean"])}
            entry["rows_mean_ms"] = round(med["rows_mean"], 4)
            entry["rows_mean_per_frame_ms"] = round(med["rows_mean"] / count, 5)
            # (3) an all-stopped frame: the stop-everything run renders two frames and count - 2 empty ones
            entry["a_frame_whose_every_tile_has_stopped_ms"] = round(
                (med["stops_everything_at_2"] - 2.0 * med["never_stops"] / count) / (count - 2), 5)
            # ... and the passes of the last launches (rtx_launch_timings: the scheduling pass with the order pass, the shading pass)
            last = min(count, 8)
            top = "middle_q%02d" % round(100 * max(self.args.middle))
            entry["passes_of_the_last_%d_launches_ms" % last] = {
                name: {"schedule_median": round(float(np.median(passes[name][0][-last:])), 5),
                       "shade_median": round(float(np.median(passes[name][1][-last:])), 5),
                       "shade_max": round(float(np.max(passes[name][1][-last:])), 5)}
                for name in ("rows_mean", "never_stops", top, "stops_everything_at_2")}
            doc["frames"].append(entry)

    def report(self, doc):
        med = {}
        doc["cases"] = []
        for name, v in self.ms.items():
            doc["cases"].append(dict(summary(v), case=name[:-3]))
            med[name] = float(np.median(v))
            print("%-52s min %9.5f ms  median %9.5f ms  spread %.3f" % (name[:-3], min(v), med[name], (max(v) - min(v)) / min(v)), file=sys.stderr)
        return med


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--batch", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--middle", type=float, nargs="+", default=[0.25, 0.5, 0.75, 0.9, 0.99], help="(2): quantiles of the tile errors, as thresholds")
    ap.add_argument("--parent", default=None, help="(4): the parent commit's tree, built")
    ap.add_argument("--bench", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    doc = {"frame": [W, H], "repeats": args.repeats, "batch": args.batch}
    b = Bench(args)
    doc["device"] = b.torch.cuda.get_device_name(0)
    b.kernel_cases()
    b.frames(doc)
    med = b.report(doc)
    # the rule that never stops: per frame not slower than the pipeline mean by more than that yardstick's own run-to-run
    # spread, the measured difference of the two adds and a device-to-device copy of the 32 extra bytes per pixel
    doc["never_stops_within_the_rows_mean"] = {}
    for count in FRAME_COUNTS:
        rows = b.ms["rows_mean_%d_frames_ms" % count]
        spread_ms = (max(rows) - min(rows)) / count
        extra = med["kernel_moment_add_ms"] - med["kernel_accum_add_ms"]
        copy = med["kernel_copy_of_32_bytes_per_pixel_ms"]
        allowed = med["rows_mean_%d_frames_ms" % count] / count + spread_ms + extra + copy
        got = med["never_stops_%d_frames_ms" % count] / count
        doc["never_stops_within_the_rows_mean"]["%d_frames" % count] = {
            "per_frame_ms": round(got, 5), "rows_mean_per_frame_ms": round(med["rows_mean_%d_frames_ms" % count] / count, 5),
            "rows_mean_spread_per_frame_ms": round(spread_ms, 5), "moment_add_minus_accum_add_ms": round(extra, 5),
            "copy_of_32_bytes_per_pixel_ms": round(copy, 5), "allowed_per_frame_ms": round(allowed, 5), "within": bool(got <= allowed)}
    # (the rule that stops everything at 2 renders two frames, not a mean of N: it is no answer to "anywhere")
    doc["beats_the_pipeline_mean_at_a_middle_threshold"] = bool(any(r["beats_the_pipeline_mean"] for e in doc["frames"]
                                                                    for name, r in e["rules"].items() if name.startswith("middle")))
    b.scene.close()
    if args.parent and args.bench:                                        # (4); who goes first alternates too
        roots = [("parent", os.path.abspath(args.parent)), ("this", HERE)]
        lines = {who: [] for who, _ in roots}
        for k in range(args.rounds):
            for who, root in roots[::-1] if k % 2 else roots:
                lines[who].append(bench_line(root))
                print("bench.py of %s, round %d: %s" % (who, k, lines[who][-1]), file=sys.stderr, flush=True)
        doc["bench"] = {"command": "bench.py --gpus 1 --steps 20 --warmup 3", **lines}
    text = json.dumps(doc, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
