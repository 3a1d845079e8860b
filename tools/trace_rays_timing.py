#!/usr/bin/env python3
"""Times rtx_trace_rays_device in the caller's order and with the regrouping pass, on two workloads built from the
1920x1080 big_bunny scene: its primary rays in pixel order (coherent: 64 neighbouring pixels of a row per wavefront) and
the same rays in a seeded random permutation (incoherent).  For each batch size n the batch is the first n rays of the
workload; times are device milliseconds between two events on the launch's stream (key kernel + radix sort + trace
kernel, uncounted form), median of --runs after --warmup.

The library skips the regrouping pass below rtxq::kRegroupMinRays (csrc/rtx_query.h).  That figure should be the smallest n
from which regrouping the shuffled workload is faster than tracing it as it comes, which this tool reports; DESIGN.md
"Ray queries" says whether the current figure has been taken from a run of it.  One JSON document on stdout, and in --out when given.

    python tools/trace_rays_timing.py --out profiles/trace_rays_timing.json
"""
import argparse
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
F = np.float32


def primary_rays(rtx, width, height, samples):
    """create_rays (main.rs:151-178) for sample 0 of every pixel, row-major pixel order; float32, not normalised"""
    u, v, w = rtx.camera_new(rtx.DEFAULT_EYE, rtx.DEFAULT_LOOK_AT, rtx.DEFAULT_UP)
    py, px = np.meshgrid(np.arange(height, dtype=np.uint32), np.arange(width, dtype=np.uint32), indexing="ij")
    k = ((px.astype(np.uint64) * width + py) % len(samples)).astype(np.int64)
    a = (px.astype(F) - F(width) / F(2) + samples[k, 0]).reshape(-1, 1)
    b = (py.astype(F) - F(height) / F(2) + samples[k, 1]).reshape(-1, 1)
    d = (a * u[None, :] + b * v[None, :] - F(rtx.DEFAULT_DISTANCE) * w[None, :]).astype(F)
    o = np.tile(np.asarray(rtx.DEFAULT_EYE, F), (len(d), 1))
    return np.ascontiguousarray(o), np.ascontiguousarray(d)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--runs", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--sizes", type=int, nargs="*", default=[1 << k for k in range(8, 21)] + [1920 * 1080])
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch  # before librtx.so: one HIP runtime per process (tests/conftest.py)
    rtx = importlib.import_module("ray-tracer-rust_amd")
    if rtx.device_count() < 1 or not torch.cuda.is_available():
        raise SystemExit("no HIP device: the ray queries have no CPU fallback")
    width, height = rtx.DEFAULT_WIDTH, rtx.DEFAULT_HEIGHT
    samples = rtx.gen_samples()
    scene = rtx.default_scene([os.path.join(ROOT, "models", "big_bunny.obj")], width, height, samples)
    o, d = primary_rays(rtx, width, height, samples)
    perm = np.random.default_rng(args.seed).permutation(len(o))
    workloads = {"pixel_order": (o, d), "shuffled": (o[perm], d[perm])}

    stream = torch.cuda.Stream(device="cuda:0")
    results = []
    reference = None
    with torch.cuda.stream(stream):
        hits = torch.zeros(len(o) * 32, dtype=torch.uint8, device="cuda:0")
        for name, (wo, wd) in workloads.items():
            t_o, t_d = torch.from_numpy(wo).to("cuda:0"), torch.from_numpy(wd).to("cuda:0")
            for n in sorted(set(min(s, len(o)) for s in args.sizes)):
                row = {"workload": name, "n_rays": n}
                for mode, kw in (("keep_order", dict(keep_order=True)), ("regrouped", dict(force_regroup=True))):
                    ms = []
                    for i in range(args.warmup + args.runs):
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        e0.record(stream)
                        scene.trace_rays_device(0, n, t_o.data_ptr(), t_d.data_ptr(), hits.data_ptr(), stream.cuda_stream, **kw)
                        e1.record(stream)
                        e1.synchronize()
                        if i >= args.warmup:
                            ms.append(e0.elapsed_time(e1))
                    row[mode + "_ms"] = round(float(np.median(ms)), 4)
                    row[mode + "_min_ms"] = round(float(np.min(ms)), 4)
                    if n == len(o):   # the whole frame: both modes, both workloads must describe the same hits
                        got = hits.cpu().numpy().view(rtx.rtx.RAY_HIT_DTYPE)
                        got = got if name == "pixel_order" else got[np.argsort(perm)]
                        reference = got.copy() if reference is None else reference
                        row[mode + "_same_hits"] = bool(got.tobytes() == reference.tobytes())
                row["speedup_regrouped"] = round(row["keep_order_ms"] / row["regrouped_ms"], 3)
                results.append(row)
                print("%-12s n=%8d  keep_order %9.4f ms  regrouped %9.4f ms  x%.2f" %
                      (name, n, row["keep_order_ms"], row["regrouped_ms"], row["speedup_regrouped"]), file=sys.stderr)
    shuffled = [r for r in results if r["workload"] == "shuffled"]
    pays = [r["n_rays"] for r in shuffled if r["regrouped_ms"] < r["keep_order_ms"]]
    never_again = [r["n_rays"] for r in shuffled if r["regrouped_ms"] >= r["keep_order_ms"]]
    doc = {"scene": "big_bunny.obj + ground, %dx%d, default camera" % (width, height), "device": torch.cuda.get_device_name(0),
           "runs": args.runs, "warmup": args.warmup, "seed": args.seed,
           "hits": int((reference["prim"] != rtx.rtx.NO_HIT).sum()) if reference is not None else None,
           "smallest_n_from_which_regrouping_always_pays_on_shuffled": min([n for n in pays if not never_again or n > max(never_again)], default=None),
           "results": results}
    text = json.dumps(doc, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    scene.close()


if __name__ == "__main__":
    main()
