#!/usr/bin/env python3
"""Times rtx_render_view_device of big_bunny's own 1920x1080 view beside the two other ways to the same frame:

    view_all               rtx_render_view_device, d_rgb + d_shade + d_hits
    view_rgb               rtx_render_view_device, d_rgb only
    shade_pixel_order      rtx_shade_rays_device with RTX_RAYS_KEEP_ORDER on the same rays in pixel order (64 x 1 strips)
    render_tiles           rtx_render_tiles_device: the render pipeline (cuts, rings, a scheduling pass)

Device time between two events on the launch's stream, uncounted kernel forms.  The cases are interleaved: --repeats
rounds of one launch each after --warmup rounds; reported are the minimum, the median and the spread (max - min) / min.
All cases must give the same frame bytes, which the tool checks.  --root DIR measures the build of ANOTHER checkout of
this repository (its package and librtx.so; a build without the view calls runs the last two cases only), which is how
the yardstick — shade_pixel_order on the parent commit's build, same session — is taken; --yardstick FILE puts such a
run's shade_pixel_order row beside this one's cases.  One JSON document on stdout, and in --out when given.

    python tools/render_view_timing.py --root ../parent --out parent.json
    python tools/render_view_timing.py --yardstick parent.json --out profiles/render_view_timing.json
"""
import argparse
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from trace_rays_timing import primary_rays  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--root", default=ROOT)
    ap.add_argument("--yardstick", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch  # before librtx.so: one HIP runtime per process (tests/conftest.py)
    root = os.path.abspath(args.root)
    sys.path.insert(0, root)
    rtx = importlib.import_module("ray-tracer-rust_amd")
    if rtx.device_count() < 1 or not torch.cuda.is_available():
        raise SystemExit("no HIP device: rendering has no CPU fallback")
    width, height = rtx.DEFAULT_WIDTH, rtx.DEFAULT_HEIGHT
    samples = rtx.gen_samples()
    scene = rtx.default_scene([os.path.join(root, "models", "big_bunny.obj")], width, height, samples)
    n = width * height
    stream = torch.cuda.Stream(device="cuda:0")
    with torch.cuda.stream(stream):
        o, d = primary_rays(rtx, width, height, samples)
        t_o, t_d = torch.from_numpy(o).to("cuda:0"), torch.from_numpy(d).to("cuda:0")
        rgb = {k: torch.zeros(n * 3, dtype=torch.uint8, device="cuda:0") for k in ("view_all", "view_rgb", "render_tiles")}
        shade = {k: torch.zeros(n * 16, dtype=torch.uint8, device="cuda:0") for k in ("view_all", "shade_pixel_order")}
        hits = torch.zeros(n * 32, dtype=torch.uint8, device="cuda:0")
        s = stream.cuda_stream
        cases = {}
        if hasattr(scene, "render_view_device"):
            own = scene.own_view()
            cases["view_all"] = lambda: scene.render_view_device(0, own, rgb["view_all"].data_ptr(), shade["view_all"].data_ptr(),
                                                                 hits.data_ptr(), s)
            cases["view_rgb"] = lambda: scene.render_view_device(0, own, rgb["view_rgb"].data_ptr(), None, None, s)
        cases["shade_pixel_order"] = lambda: scene.shade_rays_device(0, n, t_o.data_ptr(), t_d.data_ptr(),
                                                                     shade["shade_pixel_order"].data_ptr(), None, s, keep_order=True)
        cases["render_tiles"] = lambda: scene.render_tiles_device(0, 0, 1, height, rgb["render_tiles"].data_ptr(), n * 3, s)
        ms = {k: [] for k in cases}
        for i in range(args.warmup + args.repeats):
            for name, launch in cases.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                launch()
                e1.record(stream)
                e1.synchronize()
                if i >= args.warmup:
                    ms[name].append(e0.elapsed_time(e1))
        frame = rgb["render_tiles"].cpu().numpy().reshape(n, 3)
        same = {"render_tiles": True,
                "shade_pixel_order": bool(np.array_equal(shade["shade_pixel_order"].cpu().numpy().view(rtx.rtx.PIXEL_SHADE_DTYPE)["rgb8"], frame))}
        for k in ("view_all", "view_rgb"):
            if k in cases:
                same[k] = bool(np.array_equal(rgb[k].cpu().numpy().reshape(n, 3), frame))
        if "view_all" in cases:
            same["view_all"] = same["view_all"] and shade["view_all"].cpu().numpy().tobytes() == shade["shade_pixel_order"].cpu().numpy().tobytes()
    doc = {"scene": "big_bunny.obj + ground, %dx%d, default camera" % (width, height), "device": torch.cuda.get_device_name(0),
           "repeats": args.repeats, "warmup": args.warmup, "pixels": n, "cases": []}
    for name, v in ms.items():
        row = {"case": name, "min_ms": round(min(v), 4), "median_ms": round(float(np.median(v)), 4),
               "spread": round((max(v) - min(v)) / min(v), 4), "same_bytes_as_the_frame": same[name]}
        doc["cases"].append(row)
        print("%-18s min %9.4f ms  median %9.4f ms  spread %.3f  same bytes: %s" %
              (name, row["min_ms"], row["median_ms"], row["spread"], same[name]), file=sys.stderr)
    if args.yardstick:
        with open(args.yardstick) as f:
            other = json.load(f)
        doc["yardstick"] = next(r for r in other["cases"] if r["case"] == "shade_pixel_order")
        doc["yardstick"]["what"] = "shade_pixel_order on the parent commit's build, same session"
        for r in doc["cases"]:
            r["ratio_to_yardstick"] = round(r["min_ms"] / doc["yardstick"]["min_ms"], 3)
    text = json.dumps(doc, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    scene.close()
    if not all(same.values()):
        raise SystemExit("a case's bytes differ from the frame")


if __name__ == "__main__":
    main()
