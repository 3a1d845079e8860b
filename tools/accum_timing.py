#!/usr/bin/env python3
"""Times the mean of N frames kept on the device (rtx_render_view_mean_device, rtx_accum_add_device,
rtx_accum_resolve_device) on big_bunny + ground in a 1920 x 1080 frame, beside what the parent commit can do for the same
mean through this build.  Kernel times are HIP events around --batch back-to-back launches on one stream, divided by the
batch; call times are the host's clock around the calls, the stream waited for.

  (1) the accumulator kernels beside a device-to-device hipMemcpyAsync of the bytes each moves (a copy of B bytes moves 2 B:
      the yardstick of a kernel that moves M bytes is a copy of M / 2): add under `first` (16 + 16 bytes per pixel), add
      (32 + 16), resolve into records and RGB8 (16 + 19), into records alone (16 + 16), into RGB8 alone (16 + 3), the
      latter at d_rgb offsets 0 and 1.  --other-lib PATH: the resolve cases of another build of the library beside this
      one's (a kernel form under trial), in child processes, alternated --rounds times.
  (2) rtx_render_view_mean_device at 1, 4, 16 and 64 frames beside the parent's way, n x (rtx_scene_reseed +
      rtx_render_view_lit to host records + a numpy float32 sum), divided and quantised by rtxh_accum_resolve.  Every
      resolved frame is compared byte for byte.
  (3) the per-frame overhead over a bare rtx_render_view_device: the mean call's time per frame at 16 frames minus the
      view's, and its parts as differences (the add alone is (1)'s).
  (4) --parent DIR [--parent2 DIR] --bench: bench.py --gpus 1 --steps 20 --warmup 3 of the builds under DIR (the parent
      commit's tree, built; a second copy of it shows the spread of two identical builds) and of this one, alternated
      --rounds times (bench.py does not reach the new code).
  (5) --mean-path --parent DIR --parent2 DIR [--bench]: in place of (1) to (3), the host-side cost of every mean call —
      through the view kernel, through the pipeline, adaptive under a rule that never stops; device-resident and host —
      at 1, 4, 16 and 64 frames, of the three builds (each tree's own binding and library, a child process each),
      alternated --rounds times; per case, whether this build's median is as near a parent's as the two parents' are to
      each other.

--repeats interleaved rounds after --warmup rounds; reported are the minimum, the median and the spread (max - min) / min.
One JSON document on stdout, and in --out.

    python tools/accum_timing.py --parent ../parent --parent2 ../parent2 --bench --out profiles/accum_timing.json
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

    def wall(self, call):
        t0 = time.perf_counter()
        call()
        self.stream.synchronize()
        return 1e3 * (time.perf_counter() - t0)

    # ---- (1)
    def kernel_cases(self, resolve_only=False):
        sc, n, s = self.scene, self.n, self.s
        rec, acc, out = self.dev(16 * n), self.dev(16 * n), self.dev(16 * n)
        rgb = self.dev(3 * n + 16)
        sc.render_view_device(0, self.view, d_shade_ptr=rec.data_ptr(), stream=s)
        sc.accum_add_device(0, n, rec.data_ptr(), acc.data_ptr(), True, s)
        self.stream.synchronize()
        cases = {
            "resolve_records_and_rgb": (35, lambda: sc.accum_resolve_device(0, n, acc.data_ptr(), 16, rgb.data_ptr(), out.data_ptr(), s)),
            "resolve_rgb_alone": (19, lambda: sc.accum_resolve_device(0, n, acc.data_ptr(), 16, rgb.data_ptr(), None, s)),
            "resolve_rgb_alone_offset_1": (19, lambda: sc.accum_resolve_device(0, n, acc.data_ptr(), 16, rgb.data_ptr() + 1, None, s)),
            "resolve_records_alone": (32, lambda: sc.accum_resolve_device(0, n, acc.data_ptr(), 16, None, out.data_ptr(), s)),
        }
        if not resolve_only:
            cases["add_first"] = (32, lambda: sc.accum_add_device(0, n, rec.data_ptr(), acc.data_ptr(), True, s))
            cases["add"] = (48, lambda: sc.accum_add_device(0, n, rec.data_ptr(), acc.data_ptr(), False, s))
        copies = {}
        for per_pixel in sorted({b for b, _ in cases.values()}):
            half = per_pixel * n // 2
            src, dst = self.dev(half), self.dev(half)
            copies[per_pixel] = lambda src=src, dst=dst: dst.copy_(src, non_blocking=True)
        for i in range(self.args.warmup + self.args.repeats):
            for name, (per_pixel, call) in cases.items():
                t_kernel, t_copy = self.events(call), self.events(copies[per_pixel])
                if i >= self.args.warmup:
                    self.add("kernel_%s_ms" % name, t_kernel)
                    self.add("copy_of_%d_bytes_per_pixel_ms" % per_pixel, t_copy)
        return {name: per_pixel for name, (per_pixel, _) in cases.items()}

    # ---- (2), (3)
    def frames(self, doc):
        sc, rtx, n, s = self.scene, self.rtx, self.n, self.s
        n_pairs = sc.n_samples()
        own = sc.light()
        thr = sc.gamma_thresholds()
        acc, rgb, rec = self.dev(16 * n), self.dev(3 * n), self.dev(16 * n)
        doc["mean"] = []
        for count in FRAME_COUNTS:
            seeds = [1000 + k for k in range(count)]
            repeats = max(2, self.args.repeats // (1 if count <= 4 else 2 if count == 16 else 4))
            for i in range(1 + repeats):
                t_mean = self.wall(lambda: sc.render_view_mean_device(0, self.view, seeds, n_pairs, acc.data_ptr(), rgb.data_ptr(), None, s))
                got = rgb.cpu().numpy().reshape(H, W, 3)

                def parents_way():
                    total = None
                    for seed in seeds:
                        sc.reseed(seed, n_pairs)
                        _, shade = sc.render_view(self.view, want_shade=True, light=own)
                        total = rtx.accum_add(shade, total)          # (numpy's float32 sum costs the same: one pass over 33 MB)
                    return rtx.accum_resolve(thr, total, count)[0]
                t0 = time.perf_counter()
                want = parents_way()
                t_parent = 1e3 * (time.perf_counter() - t0)
                bad = int((got != want).any(axis=2).sum())
                if bad:
                    raise SystemExit("%d frames: %d pixels differ from the parent's way" % (count, bad))
                if i >= 1:
                    self.add("mean_device_%d_frames_ms" % count, t_mean)
                    self.add("parents_way_%d_frames_ms" % count, t_parent)
            doc["mean"].append({"frames": count, "differing_pixels": 0})
        sc.reseed(rtx.DEFAULT_SEED, n_pairs)
        # (3): a bare view launch, and the chain's other kernels by what the frame count 16 leaves over
        for i in range(self.args.warmup + self.args.repeats):
            t_view = self.events(lambda: sc.render_view_device(0, self.view, d_shade_ptr=rec.data_ptr(), stream=s), batch=4)
            seeds = [2000 + k for k in range(16)]
            t_chain = self.events(lambda: sc.render_view_mean_device(0, self.view, seeds, n_pairs, acc.data_ptr(), None, None, s), batch=1) / 16
            if i >= self.args.warmup:
                self.add("view_device_alone_ms", t_view)
                self.add("mean_chain_per_frame_of_16_ms", t_chain)

    def report(self, doc):
        med = {}
        doc["cases"] = []
        for name, v in self.ms.items():
            doc["cases"].append(dict(summary(v), case=name[:-3]))
            med[name] = float(np.median(v))
            print("%-44s min %9.5f ms  median %9.5f ms  spread %.3f" % (name[:-3], min(v), med[name], (max(v) - min(v)) / min(v)), file=sys.stderr)
        return med


def kernels_doc(args, resolve_only):
    b = Bench(args)
    per_pixel = b.kernel_cases(resolve_only)
    doc = {"lib": b.rtx.rtx.LIB_PATH}
    med = b.report(doc)
    doc["bandwidth"] = {}
    for name, bytes_pp in per_pixel.items():
        k, c = med["kernel_%s_ms" % name], med["copy_of_%d_bytes_per_pixel_ms" % bytes_pp]
        moved = bytes_pp * W * H
        doc["bandwidth"][name] = {"bytes_moved": moved, "kernel_GBps": round(moved / k / 1e6, 1), "copy_GBps": round(moved / c / 1e6, 1),
                                  "kernel_over_copy": round(c / k, 3)}
    b.scene.close()
    return doc


MEAN_CALL_REPEATS = {1: 41, 4: 15, 16: 5, 64: 3}


def mean_calls(root):
    """(5)'s child: the build under `root` (its binding and its library), every mean call at every frame count, the host's
    clock around the call and the wait for the stream; the samples of every case"""
    import torch  # before librtx.so: one HIP runtime per process (tests/conftest.py)
    sys.path.insert(0, root)
    rtx = importlib.import_module("ray-tracer-rust_amd")
    tris, rgb = rtx.default_primitives([os.path.join(root, "models", "big_bunny.obj")])
    sc = rtx.Scene(W, H, tris, rgb, rtx.gen_samples())
    sc.upload(0)
    view, n, n_pairs = sc.own_view(), W * H, sc.n_samples()
    stream = torch.cuda.Stream(device="cuda:0")
    s = stream.cuda_stream
    state, tiles, d_rgb = (torch.empty(b, dtype=torch.uint8, device="cuda:0").data_ptr() for b in (32 * n, 8 * ((W + 7) // 8) * ((H + 7) // 8), 3 * n))
    calls = {
        "view_mean_device": lambda sd: sc.render_view_mean_device(0, view, sd, n_pairs, state, d_rgb, None, s),
        "rows_mean_device": lambda sd: sc.render_view_mean_device(0, view, sd, n_pairs, state, d_rgb, None, s, rows=True),
        "never_stops_device": lambda sd: sc.render_view_adaptive_device(0, view, sd, (len(sd), 0.0), n_pairs, state, tiles, d_rgb, None, s),
        "view_mean_host": lambda sd: sc.render_view_mean(view, sd, n_pairs),
        "rows_mean_host": lambda sd: sc.render_view_mean(view, sd, n_pairs, rows=True),
        "never_stops_host": lambda sd: sc.render_view_adaptive(view, sd, (len(sd), 0.0), n_pairs),
    }
    ms = {}
    for count in FRAME_COUNTS:
        seeds = [1000 + k for k in range(count)]
        for i in range(1 + MEAN_CALL_REPEATS[count]):
            for name in list(calls)[::-1] if i % 2 else list(calls):
                stream.synchronize()
                t0 = time.perf_counter()
                calls[name](seeds)
                stream.synchronize()
                if i >= 1:
                    ms.setdefault("%s_%d_frames" % (name, count), []).append(1e3 * (time.perf_counter() - t0))
    sc.close()
    return {"lib": rtx.rtx.LIB_PATH, "ms": ms}


def mean_path(args, roots):
    """(5): mean_calls of every build in a child process each, --rounds times, who goes first rotating; per case the pooled
    samples' summary per build and whether this build's median is as near a parent's as the two parents' are to each other"""
    pooled = {who: {} for who, _ in roots}
    for k in range(args.rounds):
        for who, root in roots[k % len(roots):] + roots[:k % len(roots)]:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--mean-calls", root], capture_output=True, text=True, timeout=600)
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
        if "parent2" in med:
            between = abs(med["parent"] - med["parent2"])
            away = min(abs(med["this"] - med["parent"]), abs(med["this"] - med["parent2"]))
            out[case].update(parents_apart_ms=round(between, 5), this_from_nearer_parent_ms=round(away, 5), within=bool(away <= between))
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--mean-calls", default=None, metavar="ROOT", help="(5)'s child: the mean calls of the build under ROOT")
    ap.add_argument("--mean-path", action="store_true", help="(5) and, with --bench, (4) alone")
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--batch", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--other-lib", default=None, help="(1): another build of the library, its resolve cases beside this one's")
    ap.add_argument("--resolve-only", action="store_true", help="(1)'s resolve cases of the library in RTX_PY_LIB, as a child of --other-lib")
    ap.add_argument("--parent", default=None, help="(4): the parent commit's tree, built")
    ap.add_argument("--parent2", default=None, help="(4): a second copy of it")
    ap.add_argument("--bench", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.resolve_only:
        print(json.dumps(kernels_doc(args, True)))
        return
    if args.mean_calls:
        print(json.dumps(mean_calls(os.path.abspath(args.mean_calls))))
        return
    roots = [(who, os.path.abspath(root)) for who, root in (("parent", args.parent), ("this", HERE), ("parent2", args.parent2)) if root]
    doc = {"frame": [W, H], "repeats": args.repeats, "warmup": args.warmup, "batch": args.batch}
    if args.mean_path:
        doc = {"frame": [W, H], "rounds": args.rounds, "samples_per_round": MEAN_CALL_REPEATS, "mean_calls": mean_path(args, roots)}
    else:
        measure_this_build(args, doc)
    if args.parent and args.bench:                                        # (4); who goes first alternates too
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


def measure_this_build(args, doc):
    """(1), (2), (3)"""
    if args.other_lib:                                                   # before this process opens the device
        forms = {"this_build": None, "other_form": os.path.abspath(args.other_lib)}
        doc["resolve_forms"] = {who: [] for who in forms}
        for k in range(args.rounds):
            for who in list(forms)[::-1] if k % 2 else list(forms):
                env = dict(os.environ)
                if forms[who]:
                    env["RTX_PY_LIB"] = forms[who]
                r = subprocess.run([sys.executable, os.path.abspath(__file__), "--resolve-only", "--repeats", str(args.repeats), "--warmup",
                                    str(args.warmup), "--batch", str(args.batch)], capture_output=True, text=True, env=env, timeout=600)
                if r.returncode != 0:
                    raise SystemExit("child for %s failed (%d):\n%s" % (who, r.returncode, (r.stdout + r.stderr)[-3000:]))
                child = json.loads(r.stdout.splitlines()[-1])
                doc["resolve_forms"][who].append({"lib": child["lib"], "cases": child["cases"], "bandwidth": child["bandwidth"]})
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
    doc["differences_of_medians"] = {
        "per_frame_overhead_over_a_bare_view_ms": round(med["mean_chain_per_frame_of_16_ms"] - med["view_device_alone_ms"], 5),
        "of_which_add_ms": round(med["kernel_add_ms"], 5)}
    for count in FRAME_COUNTS:
        doc["differences_of_medians"]["parents_way_over_mean_device_%d_frames" % count] = round(
            med["parents_way_%d_frames_ms" % count] / med["mean_device_%d_frames_ms" % count], 2)
    b.scene.close()


if __name__ == "__main__":
    main()
