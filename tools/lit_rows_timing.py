#!/usr/bin/env python3
"""Times rtx_render_view_rows_lit_device — any view under any light through the render pipeline — on big_bunny 1920x1080
beside what it is measured against:

    (1) view_rows_own        rtx_render_view_rows_device, the scene's own view, its eye already aimed: the yardstick.  With
                             --only-unlit nothing else runs, which every build that has the call can do: --root DIR
                             measures ANOTHER checkout's package and librtx.so, how the parent commit's build is measured
                             in the same session, alternated with this one's (parent, this, parent, this ...: one process
                             each, since a process holds one librtx.so); --alternated FILE ... puts those runs' rows
                             beside this run's
        view_rows_lit_own    rtx_render_view_rows_lit_device under the scene's own light and count: the same kernels and
                             frame, the light kernels added, the tour the f32 statement's
    (2) per orbit light (the scene's light turned around the y axis, 45 / 135 / 225 / 315 degrees, 100 samples):
        view_rows_lit_lightN rtx_render_view_rows_lit_device, the light kernels included
        view_lit_lightN      rtx_render_view_lit_device, rgb only: what a caller has without the feature
        fresh_lightN         rtx_render_view_rows_device of a fresh scene created with that light, with the host time of
                             rtx_scene_create and of the upload: the other alternative
    (3) strip_lit / strip_unlit   an 8-row strip of the own view, lit (own light) against unlit: the difference is the light
                             kernels alone (both launch the whole pipeline on the same rows)

Device time between two events on the launch's stream, uncounted kernel forms.  The cases are interleaved: --repeats rounds
of one launch each after --warmup rounds; reported are the minimum, the median and the spread (max - min) / min.  Every lit
frame is compared with rtx_render_view_lit's bytes of the same view and light before a time is recorded.  One JSON
document on stdout, and in --out when given.

    python tools/lit_rows_timing.py --root ../parent --label parent --only-unlit --out parent_1.json
    python tools/lit_rows_timing.py --only-unlit --out this_1.json          (and so on, alternating)
    python tools/lit_rows_timing.py --alternated parent_1.json this_1.json ... --out profiles/lit_rows_timing.json
"""
import argparse
import importlib
import json
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ANGLES = (45, 135, 225, 315)
STRIP_ROWS = 8


def turned(tri, deg):
    """a triangle (nine floats) turned by `deg` around the y axis"""
    c, s = math.cos(math.radians(deg)), math.sin(math.radians(deg))
    t = np.asarray(tri, np.float64).reshape(3, 3)
    return tuple(float(x) for x in np.stack([t[:, 0] * c + t[:, 2] * s, t[:, 1], -t[:, 0] * s + t[:, 2] * c], axis=1).reshape(9))


def row(name, v, **more):
    out = {"case": name, "min_ms": round(min(v), 4), "median_ms": round(float(np.median(v)), 4),
           "spread": round((max(v) - min(v)) / min(v), 4)}
    out.update(more)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--root", default=ROOT)
    ap.add_argument("--label", default="this", help="names the build in the document (the parent's runs: parent)")
    ap.add_argument("--only-unlit", action="store_true")
    ap.add_argument("--alternated", nargs="*", default=[])
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch  # before librtx.so: one HIP runtime per process (tests/conftest.py)
    sys.path.insert(0, os.path.abspath(args.root))
    rtx = importlib.import_module("ray-tracer-rust_amd")
    if rtx.device_count() < 1 or not torch.cuda.is_available():
        raise SystemExit("no HIP device: rendering has no CPU fallback")
    width, height = rtx.DEFAULT_WIDTH, rtx.DEFAULT_HEIGHT
    n = width * height
    samples = rtx.gen_samples()
    tris, rgb_in = rtx.default_primitives([os.path.join(ROOT, "models", "big_bunny.obj")])
    scene = rtx.Scene(width, height, tris, rgb_in, samples)
    own_view, own_light = scene.own_view(), scene.light()
    lit = not args.only_unlit
    if lit and "rtx_render_view_rows_lit_device" not in rtx.rtx._SIGS:
        raise SystemExit("this build has no rtx_render_view_rows_lit_device: --only-unlit")
    count = own_light.nb_light_sample
    own_tri = list(own_light.v0) + list(own_light.v1) + list(own_light.v2)
    lights = {a: rtx.Scene.make_light(turned(own_tri, a), count) for a in ANGLES} if lit else {}
    strip = rtx.Scene.view(width, height, rect=(0, (height - STRIP_ROWS) // 2, width, STRIP_ROWS), eye=rtx.DEFAULT_EYE,
                           look_at=rtx.DEFAULT_LOOK_AT)
    fresh, create_ms, upload_ms = {}, {}, {}
    for a in lights:
        t0 = time.perf_counter()
        fresh[a] = rtx.Scene(width, height, tris, rgb_in, samples, light_tri=turned(own_tri, a))
        t1 = time.perf_counter()
        fresh[a].upload(0)
        create_ms[a], upload_ms[a] = (t1 - t0) * 1e3, (time.perf_counter() - t1) * 1e3
    stream = torch.cuda.Stream(device="cuda:0")
    doc = {"scene": "big_bunny.obj + ground, %dx%d" % (width, height), "device": torch.cuda.get_device_name(0),
           "build": args.label, "repeats": args.repeats, "warmup": args.warmup, "pixels": n,
           "nb_light_sample": count, "orbit_lights": {str(a): turned(own_tri, a) for a in lights}, "cases": []}
    same = {}
    with torch.cuda.stream(stream):
        s = stream.cuda_stream
        buf = {}

        def out(name, bytes_=n * 3):
            buf[name] = torch.zeros(bytes_, dtype=torch.uint8, device="cuda:0")
            return buf[name].data_ptr()

        cases, expect = {}, {}
        p = out("view_rows_own")
        cases["view_rows_own"] = lambda p=p: scene.render_view_rows_device(0, own_view, p, n * 3, s)
        if lit:
            p = out("view_rows_lit_own")
            cases["view_rows_lit_own"] = lambda p=p: scene.render_view_rows_device(0, own_view, p, n * 3, s, light=own_light)
            expect["view_rows_lit_own"] = None
            for a in ANGLES:
                p = out("view_rows_lit_light%d" % a)
                cases["view_rows_lit_light%d" % a] = lambda p=p, a=a: scene.render_view_rows_device(0, own_view, p, n * 3, s, light=lights[a])
                p = out("view_lit_light%d" % a)
                cases["view_lit_light%d" % a] = lambda p=p, a=a: scene.render_view_device(0, own_view, p, None, None, s, light=lights[a])
                p = out("fresh_light%d" % a)
                cases["fresh_light%d" % a] = lambda p=p, a=a: fresh[a].render_view_rows_device(0, own_view, p, n * 3, s)
                for k in ("view_rows_lit_light%d", "view_lit_light%d", "fresh_light%d"):
                    expect[k % a] = a
            sb = STRIP_ROWS * width * 3
            p = out("strip_unlit", sb)
            cases["strip_unlit"] = lambda p=p: scene.render_view_rows_device(0, strip, p, sb, s)
            p = out("strip_lit", sb)
            cases["strip_lit"] = lambda p=p: scene.render_view_rows_device(0, strip, p, sb, s, light=own_light)
        scene.render_view_rows_device(0, own_view, buf["view_rows_own"].data_ptr(), n * 3, s)      # the eye is aimed once
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
        frames = {None: scene.render_view(own_view).reshape(n, 3)}
        for a in lights:
            frames[a] = scene.render_view(own_view, light=lights[a]).reshape(n, 3)               # rtx_render_view_lit's bytes
        same["view_rows_own"] = bool(np.array_equal(buf["view_rows_own"].cpu().numpy().reshape(n, 3), frames[None]))
        for k, a in expect.items():
            same[k] = bool(np.array_equal(buf[k].cpu().numpy().reshape(n, 3), frames[a]))
        if lit:
            y0 = (height - STRIP_ROWS) // 2
            want = frames[None].reshape(height, width, 3)[y0:y0 + STRIP_ROWS].reshape(-1)
            for k in ("strip_unlit", "strip_lit"):
                same[k] = bool(np.array_equal(buf[k].cpu().numpy(), want))
        for name, v in ms.items():
            more = {"same_bytes_as_render_view": same[name]}
            if name.startswith("fresh_light"):
                a = int(name[len("fresh_light"):])
                more["host_scene_create_ms"], more["host_upload_ms"] = round(create_ms[a], 1), round(upload_ms[a], 1)
            doc["cases"].append(row(name, v, **more))
    by = {r["case"]: r for r in doc["cases"]}
    if lit:
        doc["light_kernels_ms"] = round(by["strip_lit"]["median_ms"] - by["strip_unlit"]["median_ms"], 4)
        doc["lit_own_minus_unlit_ms"] = round(by["view_rows_lit_own"]["median_ms"] - by["view_rows_own"]["median_ms"], 4)
        doc["per_light"] = [{"light": a,
                             "view_rows_lit_ms": by["view_rows_lit_light%d" % a]["median_ms"],
                             "view_lit_ms": by["view_lit_light%d" % a]["median_ms"],
                             "view_lit_over_view_rows_lit": round(by["view_lit_light%d" % a]["median_ms"] / by["view_rows_lit_light%d" % a]["median_ms"], 2),
                             "fresh_scene_total_ms": round(by["fresh_light%d" % a]["median_ms"] + create_ms[a] + upload_ms[a], 1)}
                            for a in ANGLES]
    if args.alternated:
        runs = []
        for path in args.alternated:
            with open(path) as f:
                other = json.load(f)
            r = next(x for x in other["cases"] if x["case"] == "view_rows_own")
            runs.append({"file": os.path.basename(path), "build": other["build"], "median_ms": r["median_ms"], "min_ms": r["min_ms"],
                         "spread": r["spread"]})
        doc["alternated_view_rows_own"] = runs
        groups = {}
        for r in runs:
            groups.setdefault(r["build"], []).append(r["median_ms"])
        doc["alternated_summary"] = [{"build": b, "runs": len(v), "median_of_medians_ms": round(float(np.median(v)), 4),
                                      "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)} for b, v in groups.items()]
    for r in doc["cases"]:
        print(json.dumps(r), file=sys.stderr)
    text = json.dumps(doc, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    for sc in list(fresh.values()) + [scene]:
        sc.close()
    if not all(same.values()):
        raise SystemExit("a case's bytes differ from rtx_render_view's: %s" % [k for k, v in same.items() if not v])


if __name__ == "__main__":
    main()
