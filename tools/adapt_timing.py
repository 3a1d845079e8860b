#!/usr/bin/env python3
"""Times the adaptive mean of N frames (rtx_render_view_adaptive_device, rtx_moment_add_device, rtx_moment_resolve_device) on
big_bunny + ground in a 1920 x 1080 frame.  The yardsticks are this build's rtx_render_view_mean_device and
rtx_render_view_rows_mean_device at the same N, alternated with the call under test in one run.  Call times are HIP events
around one call on a stream of its own; kernel times are events around --batch back-to-back launches, divided by the batch.

  (1) the moment kernels beside a device-to-device hipMemcpyAsync of the bytes each moves (a copy of B bytes moves 2 B: the
      yardstick of a kernel that moves M bytes is a copy of M / 2): add under `first` with tile states (16 + 32 bytes per
      pixel), add (16 + 32 + 32), add without tile states, an add whose every tile is stopped, resolve into records and RGB8
      (32 + 19), into RGB8 alone (32 + 3); and rtx_accum_add_device (16 + 16 + 16) for the difference.
  (2) at 16 and 64 frames, per round: the view mean, the pipeline mean, the adaptive call under the rule that never stops
      (min_frames = N), under a rule that stops everything at 2 (max_variance = +infinity), and under --middle thresholds
      taken from the tile errors the never-stopping run leaves (their quantiles over the tiles whose error is not 0).  For
      each: the share of tile-frames rendered (from the tile states), the time, the ratio to both yardsticks.  With
      min_frames = N the outputs, sums and hit counts are compared word for word with the view mean's.
  (3) --parent DIR --bench: bench.py --gpus 1 --steps 20 --warmup 3 of the build under DIR (the parent commit's tree, built)
      and of this one, alternated --rounds times (bench.py does not reach the new code).

--repeats interleaved rounds after --warmup rounds; reported are the minimum, the median and the spread (max - min) / min.
One JSON document on stdout, and in --out.

    python tools/adapt_timing.py --parent build_ab/parent --bench --out profiles/adapt_timing.json
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
        rec, mom, acc, out = self.dev(16 * n), self.dev(32 * n), self.dev(16 * n), self.dev(16 * n)
        tiles, stopped = self.dev(8 * self.n_tiles), self.dev(8 * self.n_tiles)
        rgb = self.dev(3 * n + 16)
        never, always = (1 << 20, 0.0), (1, INF)
        sc.render_view_device(0, self.view, d_shade_ptr=rec.data_ptr(), stream=s)
        sc.moment_add_device(0, W, H, rec.data_ptr(), mom.data_ptr(), tiles.data_ptr(), True, never, s)
        sc.moment_add_device(0, W, H, rec.data_ptr(), mom.data_ptr(), stopped.data_ptr(), True, never, s)      # states {1, +0.0}
        sc.accum_add_device(0, n, rec.data_ptr(), acc.data_ptr(), True, s)
        self.stream.synchronize()
        P = lambda t: t.data_ptr()
        cases = {
            "moment_add_first": (48, lambda: sc.moment_add_device(0, W, H, P(rec), P(mom), P(tiles), True, never, s)),
            "moment_add": (80, lambda: sc.moment_add_device(0, W, H, P(rec), P(mom), P(tiles), False, never, s)),
            "moment_add_without_tiles": (80, lambda: sc.moment_add_device(0, W, H, P(rec), P(mom), None, False, None, s)),
            "moment_add_every_tile_stopped": (0, lambda: sc.moment_add_device(0, W, H, P(rec), P(mom), P(stopped), False, always, s)),
            "moment_resolve_records_and_rgb": (51, lambda: sc.moment_resolve_device(0, n, P(mom), P(rgb), P(out), s)),
            "moment_resolve_rgb_alone": (35, lambda: sc.moment_resolve_device(0, n, P(mom), P(rgb), None, s)),
            "accum_add": (48, lambda: sc.accum_add_device(0, n, P(rec), P(acc), False, s)),
        }
        copies = {}
        for per_pixel in sorted({b for b, _ in cases.values() if b} | {32}):      # 32: the extra bytes of a moment add over the mean's add
            half = per_pixel * n // 2
            src, dst = self.dev(half), self.dev(half)
            copies[per_pixel] = lambda src=src, dst=dst: dst.copy_(src, non_blocking=True)
        for i in range(self.args.warmup + self.args.repeats):
            for name, (per_pixel, call) in cases.items():
                t_kernel = self.events(call)
                if i >= self.args.warmup:
                    self.add("kernel_%s_ms" % name, t_kernel)
            for per_pixel, copy in copies.items():
                t_copy = self.events(copy)
                if i >= self.args.warmup:
                    self.add("copy_of_%d_bytes_per_pixel_ms" % per_pixel, t_copy)
        return {name: per_pixel for name, (per_pixel, _) in cases.items() if per_pixel}

    # ---- (2)
    def frames(self, doc):
        sc, rtx, n, s = self.scene, self.rtx, self.n, self.s
        n_pairs = sc.n_samples()
        acc, mom, tiles = self.dev(16 * n), self.dev(32 * n), self.dev(8 * self.n_tiles)
        rgb, rgb2, shade, shade2 = self.dev(3 * n), self.dev(3 * n), self.dev(16 * n), self.dev(16 * n)
        P = lambda t: t.data_ptr()
        doc["frames"] = []
        for count in FRAME_COUNTS:
            seeds = [3000 + k for k in range(count)]
            mean = lambda rows: sc.render_view_mean_device(0, self.view, seeds, n_pairs, P(acc), P(rgb2), P(shade2), s, rows=rows)
            adaptive = lambda rule: sc.render_view_adaptive_device(0, self.view, seeds, rule, n_pairs, P(mom), P(tiles), P(rgb), P(shade), s)
            # the never-stopping run against the view mean, word for word; its tile errors give the middle thresholds
            self.events(lambda: mean(False), batch=1)
            self.events(lambda: adaptive((count, 0.0)), batch=1)
            self.stream.synchronize()
            m = mom.cpu().numpy().view(rtx.MOMENT_PIXEL_DTYPE)
            a = acc.cpu().numpy().view(rtx.ACCUM_PIXEL_DTYPE)
            same = (m["sum"].tobytes() == a["sum"].tobytes() and np.array_equal(m["hit_frames"], a["hit_frames"])
                    and bool(self.torch.equal(rgb, rgb2)) and bool(self.torch.equal(shade, shade2)))
            if not same:
                raise SystemExit("%d frames: min_frames = N differs from rtx_render_view_mean_device" % count)
            err = self.tiles_of(tiles)["err"]
            quantiles = [float(q) for q in np.quantile(err[err > 0], self.args.middle)]
            rules = {"never_stops": (count, 0.0), "stops_everything_at_2": (2, INF)}
            for q, thr in zip(self.args.middle, quantiles):
                rules["middle_q%02d" % round(100 * q)] = (2, thr)
            order = ["view_mean", "rows_mean"] + list(rules)
            repeats = max(3, self.args.repeats // (1 if count <= 16 else 2))
            share = {}
            for i in range(1 + repeats):
                for name in order[::-1] if i % 2 else order:
                    if name == "view_mean":
                        t = self.events(lambda: mean(False), batch=1)
                    elif name == "rows_mean":
                        t = self.events(lambda: mean(True), batch=1)
                    else:
                        t = self.events(lambda: adaptive(rules[name]), batch=1)
                        share[name] = float(self.tiles_of(tiles)["frames"].astype(np.float64).sum() / (self.n_tiles * count))
                    if i >= 1:
                        self.add("%s_%d_frames_ms" % (name, count), t)
            entry = {"frames": count, "equal_to_the_view_mean_with_min_frames_n": True, "rules": {}}
            med = {name: float(np.median(self.ms["%s_%d_frames_ms" % (name, count)])) for name in order}
            for name, rule in rules.items():
                entry["rules"][name] = {"min_frames": rule[0], "max_variance": rule[1] if rule[1] != INF else "inf",
                                        "share_of_tile_frames_rendered": round(share[name], 4), "median_ms": round(med[name], 4),
                                        "per_frame_ms": round(med[name] / count, 5),
                                        "over_view_mean": round(med[name] / med["view_mean"], 4),
                                        "over_rows_mean": round(med[name] / med["rows_mean"], 4),
                                        "beats_the_pipeline_mean": bool(med[name] < med["rows_mean"])}
            entry["view_mean_per_frame_ms"] = round(med["view_mean"] / count, 5)
            entry["rows_mean_per_frame_ms"] = round(med["rows_mean"] / count, 5)
            entry["a_frame_whose_every_wavefront_returns_at_once_ms"] = round(
                (med["stops_everything_at_2"] - 2.0 * med["never_stops"] / count) / (count - 2), 5)
            doc["frames"].append(entry)

    def report(self, doc):
        med = {}
        doc["cases"] = []
        for name, v in self.ms.items():
            doc["cases"].append(dict(summary(v), case=name[:-3]))
            med[name] = float(np.median(v))
            print("%-44s min %9.5f ms  median %9.5f ms  spread %.3f" % (name[:-3], min(v), med[name], (max(v) - min(v)) / min(v)), file=sys.stderr)
        return med


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--batch", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--middle", type=float, nargs="+", default=[0.25, 0.5, 0.75, 0.9, 0.99], help="(2): quantiles of the tile errors, as thresholds")
    ap.add_argument("--parent", default=None, help="(3): the parent commit's tree, built")
    ap.add_argument("--bench", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    doc = {"frame": [W, H], "repeats": args.repeats, "warmup": args.warmup, "batch": args.batch}
    b = Bench(args)
    doc["device"] = b.torch.cuda.get_device_name(0)
    per_pixel = b.kernel_cases()
    b.frames(doc)
    med = b.report(doc)
    doc["bandwidth"] = {}
    for name, bytes_pp in per_pixel.items():
        k, c = med["kernel_%s_ms" % name], med["copy_of_%d_bytes_per_pixel_ms" % bytes_pp]
        moved = bytes_pp * W * H
        doc["bandwidth"][name] = {"bytes_moved": moved, "kernel_GBps": round(moved / k / 1e6, 1), "copy_GBps": round(moved / c / 1e6, 1),
                                  "kernel_over_copy": round(c / k, 3)}
    # the rule that never stops: not slower per frame than the view mean by more than that yardstick's own run-to-run spread
    # plus a device-to-device copy of the 32 extra bytes per pixel the add moves
    doc["never_stops_within_the_view_mean"] = {}
    for count in FRAME_COUNTS:
        view = b.ms["view_mean_%d_frames_ms" % count]
        spread_ms = (max(view) - min(view)) / count
        extra = med["kernel_moment_add_ms"] - med["kernel_accum_add_ms"]
        allowed = med["view_mean_%d_frames_ms" % count] / count + spread_ms + med["copy_of_32_bytes_per_pixel_ms"]
        got = med["never_stops_%d_frames_ms" % count] / count
        doc["never_stops_within_the_view_mean"]["%d_frames" % count] = {
            "per_frame_ms": round(got, 5), "view_mean_per_frame_ms": round(med["view_mean_%d_frames_ms" % count] / count, 5),
            "view_mean_spread_per_frame_ms": round(spread_ms, 5), "copy_of_32_bytes_per_pixel_ms": round(med["copy_of_32_bytes_per_pixel_ms"], 5),
            "moment_add_minus_accum_add_ms": round(extra, 5), "allowed_per_frame_ms": round(allowed, 5), "within": bool(got <= allowed)}
    # (the rule that stops everything at 2 renders two frames, not a mean of N: it is no answer to "anywhere")
    doc["beats_the_pipeline_mean_at_a_middle_threshold"] = bool(any(r["beats_the_pipeline_mean"] for e in doc["frames"]
                                                                    for name, r in e["rules"].items() if name.startswith("middle")))
    b.scene.close()
    if args.parent and args.bench:                                        # (3); who goes first alternates too
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
