#!/usr/bin/env python3
"""Times relighting on big_bunny's own 1920x1080 view: rtx_render_view_lit_device beside the ways to the same frame that
need no lit call.

    view_unlit             rtx_render_view_device, d_rgb only: the scene's own light, no light kernel
    view_lit_own           rtx_render_view_lit_device with rtx_scene_light's value: the same frame, the light kernel ahead
    view_lit_orbit_K       rtx_render_view_lit_device under light K of four on a circle above the bunny (the scene's count)
    fresh_scene_orbit_K    the same frame the old way: rtx_scene_create with that light + rtx_scene_upload (host wall time,
                           create_upload_ms) and rtx_render_view_device on the new scene (device time)
    tile_unlit, tile_lit   one 8 x 1 strip of the view, unlit and lit: the light kernel alone is the difference of the two
                           medians (its launch included; the ABI exposes no event pair around the kernel itself)

Device time between two events on the launch's stream, uncounted kernel forms.  The cases are interleaved: --repeats
rounds of one launch each after --warmup rounds; reported are the minimum, the median and the spread (max - min) / min.
view_lit_own must give view_unlit's bytes and every view_lit_orbit_K its fresh scene's, which the tool checks.
--root DIR measures the build of ANOTHER checkout of this repository (its package and librtx.so; a build without the lit
calls runs view_unlit, the fresh scenes and tile_unlit only), which is how the yardstick — view_unlit on the parent
commit's build, same session — is taken; --yardstick FILE... puts such runs' view_unlit rows beside this one's cases, and
--earlier FILE... the view_unlit / view_lit_own rows of earlier runs of this build, so that runs alternated in one session
show the run-to-run spread.  One JSON document on stdout, and in --out when given.

    python tools/relight_timing.py --root ../parent --out parent_1.json
    python tools/relight_timing.py --out this_1.json
    python tools/relight_timing.py --root ../parent --out parent_2.json
    python tools/relight_timing.py --yardstick parent_1.json parent_2.json --earlier this_1.json --out profiles/relight_timing.json
"""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ORBIT_DEGREES = (35.0, 125.0, 215.0, 305.0)


def orbit_light(deg):
    """a 24-unit triangle 270 above the ground on a circle of radius 260 around the bunny"""
    a = np.deg2rad(deg)
    x, z = float(-15.0 + 260.0 * np.cos(a)), float(260.0 * np.sin(a))
    return (x - 12.0, 270.0, z - 12.0, x + 12.0, 270.0, z - 12.0, x, 290.0, z + 12.0)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--root", default=ROOT)
    ap.add_argument("--yardstick", nargs="*", default=[])
    ap.add_argument("--earlier", nargs="*", default=[])
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
    tris, rgb_of = rtx.default_primitives([os.path.join(root, "models", "big_bunny.obj")])
    scene = rtx.Scene(width, height, tris, rgb_of, samples)
    lit_build = hasattr(scene, "light")
    n = width * height
    lights = [orbit_light(d) for d in ORBIT_DEGREES]
    stream = torch.cuda.Stream(device="cuda:0")
    with torch.cuda.stream(stream):
        s = stream.cuda_stream
        own = scene.own_view()
        strip = scene.own_view()
        strip.x0, strip.y0, strip.nx, strip.ny = width // 2 - 4, height // 2, 8, 1
        buf = {}

        def out(name, size=n * 3):
            buf[name] = torch.zeros(size, dtype=torch.uint8, device="cuda:0")
            return buf[name].data_ptr()

        cases = {"view_unlit": (lambda p=out("view_unlit"): scene.render_view_device(0, own, p, None, None, s))}
        if lit_build:
            own_light = scene.light()
            cases["view_lit_own"] = lambda p=out("view_lit_own"): scene.render_view_device(0, own, p, None, None, s, light=own_light)
            for k, tri in enumerate(lights):
                cases["view_lit_orbit_%d" % k] = lambda p=out("view_lit_orbit_%d" % k), l=rtx.Scene.make_light(tri): \
                    scene.render_view_device(0, own, p, None, None, s, light=l)
            cases["tile_lit"] = lambda p=out("tile_lit", 24): scene.render_view_device(0, strip, p, None, None, s, light=own_light)
        cases["tile_unlit"] = lambda p=out("tile_unlit", 24): scene.render_view_device(0, strip, p, None, None, s)
        for k in range(len(lights)):
            out("fresh_scene_orbit_%d" % k)
        ms = {k: [] for k in cases}
        ms.update({"fresh_scene_orbit_%d" % k: [] for k in range(len(lights))})
        create_ms = {k: [] for k in range(len(lights))}

        def timed(launch):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            launch()
            e1.record(stream)
            e1.synchronize()
            return e0.elapsed_time(e1)

        for i in range(args.warmup + args.repeats):
            for name, launch in cases.items():
                t = timed(launch)
                if i >= args.warmup:
                    ms[name].append(t)
            for k, tri in enumerate(lights):               # the old way: a scene per light
                name = "fresh_scene_orbit_%d" % k
                t0 = time.perf_counter()
                fresh = rtx.Scene(width, height, tris, rgb_of, samples, light_tri=tri)
                fresh.upload(0)
                t1 = time.perf_counter()
                fresh.render_view_device(0, own, buf[name].data_ptr(), None, None, s)      # (first launch on a new scene)
                stream.synchronize()
                t = timed(lambda: fresh.render_view_device(0, own, buf[name].data_ptr(), None, None, s))
                fresh.close()
                if i >= args.warmup:
                    ms[name].append(t)
                    create_ms[k].append((t1 - t0) * 1e3)
        frame = buf["view_unlit"].cpu().numpy()
        same = {"view_unlit": True, "tile_unlit": True}
        for k in range(len(lights)):
            same["fresh_scene_orbit_%d" % k] = bool((buf["fresh_scene_orbit_%d" % k].cpu().numpy() != frame).any())   # another light: another frame
        if lit_build:
            same["view_lit_own"] = bool(np.array_equal(buf["view_lit_own"].cpu().numpy(), frame))
            same["tile_lit"] = bool(np.array_equal(buf["tile_lit"].cpu().numpy(), buf["tile_unlit"].cpu().numpy()))
            for k in range(len(lights)):
                same["view_lit_orbit_%d" % k] = bool(np.array_equal(buf["view_lit_orbit_%d" % k].cpu().numpy(),
                                                                    buf["fresh_scene_orbit_%d" % k].cpu().numpy()))
    doc = {"scene": "big_bunny.obj + ground, %dx%d, default camera, rgb only" % (width, height), "device": torch.cuda.get_device_name(0),
           "root": "this checkout" if root == ROOT else "another checkout (--root)", "lit_calls": lit_build,
           "repeats": args.repeats, "warmup": args.warmup, "pixels": n, "orbit_degrees": list(ORBIT_DEGREES), "cases": []}
    for name, v in ms.items():
        row = {"case": name, "min_ms": round(min(v), 4), "median_ms": round(float(np.median(v)), 4),
               "spread": round((max(v) - min(v)) / min(v), 4), "bytes_as_expected": same[name]}
        if name.startswith("fresh_scene_orbit_"):
            c = create_ms[int(name.rsplit("_", 1)[1])]
            row["create_upload_ms"] = {"min": round(min(c), 2), "median": round(float(np.median(c)), 2)}
        doc["cases"].append(row)
        print("%-22s min %9.4f ms  median %9.4f ms  spread %.3f  bytes as expected: %s" %
              (name, row["min_ms"], row["median_ms"], row["spread"], same[name]), file=sys.stderr)
    by = {r["case"]: r for r in doc["cases"]}
    if lit_build:
        doc["light_kernel_alone_ms"] = round(by["tile_lit"]["median_ms"] - by["tile_unlit"]["median_ms"], 4)
    doc["yardstick"], doc["earlier_runs"] = [], []
    for path, into, keep in [(p, doc["yardstick"], ("view_unlit",)) for p in args.yardstick] + \
                            [(p, doc["earlier_runs"], ("view_unlit", "view_lit_own")) for p in args.earlier]:
        with open(path) as f:
            other = json.load(f)
        into.append({"run": os.path.basename(path), "cases": [r for r in other["cases"] if r["case"] in keep]})
    if doc["yardstick"] and lit_build:
        # the expectation: a lit view with the scene's own light costs what the parent's rtx_render_view_device costs, within
        # the light kernel plus the spread this session shows — of the parent's own runs and inside each run
        parent = [r for run in doc["yardstick"] for r in run["cases"]]
        medians = [r["median_ms"] for r in parent]
        noise = (max(medians) - min(medians)) + max(r["spread"] * r["min_ms"] for r in parent + [by["view_lit_own"]])
        excess = by["view_lit_own"]["median_ms"] - float(np.median(medians))
        doc["expectation"] = {"what": "view_lit_own median - the parent's view_unlit median <= the light kernel alone + the spread observed",
                              "excess_ms": round(excess, 4), "light_kernel_alone_ms": doc["light_kernel_alone_ms"],
                              "spread_observed_ms": round(noise, 4),
                              "holds": bool(excess <= max(doc["light_kernel_alone_ms"], 0.0) + noise)}
    text = json.dumps(doc, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    scene.close()
    if not all(same.values()):
        raise SystemExit("a case's bytes are not what they should be")


if __name__ == "__main__":
    main()
