#!/usr/bin/env python3
"""Times rtx_render_view_rows_device — any view through the render pipeline — on big_bunny 1920x1080 beside what it is
measured against:

    (a) tiles_own            rtx_render_tiles_device, the scene's own camera: the yardstick
    (b) view_rows_own        rtx_render_view_rows_device, the scene's own view, its eye already aimed (an untimed call of
                             the same view goes first): the same kernels, one pointer apart
    (c) per orbit eye (the camera's height and radius around the y axis, 0 / 90 / 180 / 270 degrees, 0 = the own camera):
        view_rows_eyeN       rtx_render_view_rows_device, the aim kernels included (the buffer holds another eye before)
        view_eyeN            rtx_render_view_device, rgb only: the plain view kernel
        tiles_fresh_eyeN     rtx_render_tiles_device of a fresh scene created with that eye, and the host time of
                             creating it: what the feature replaces
    (d) aim_*                the two aim kernels alone, as the difference of two launches of a one-row, eight-pixel view:
                             eyes alternating (the kernels run) minus one eye repeated (they do not); on big_bunny and on
                             the 1M-triangle rtxh_synthetic_mesh scene (RTX_REFTREE_NEVER; --no-1m leaves it out)
    (e) schedule_ms / shade_ms of rtx_launch_timings for (c)'s view_rows launches

Device time between two events on the launch's stream, uncounted kernel forms.  The cases are interleaved: --repeats
rounds of one launch each after --warmup rounds; reported are the minimum, the median and the spread (max - min) / min.
Every frame is compared with rtx_render_view's bytes of the same view before a time is recorded.  --root DIR measures the
build of ANOTHER checkout's package and librtx.so (a build without rtx_render_view_rows runs (a) and (c)'s view_eyeN
only): how the yardstick rows are taken on the parent commit's build in the same session; --yardstick FILE puts that
run's rows beside this one's.  One JSON document on stdout, and in --out when given.

    python tools/view_rows_timing.py --root ../parent --out parent.json
    python tools/view_rows_timing.py --yardstick parent.json --out profiles/view_rows_timing.json
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
ANGLES = (0, 90, 180, 270)


def orbit(rtx, deg):
    """eye and look_at of the default camera turned by `deg` around the y axis (0: the default camera itself)"""
    (ex, ey, ez), (lx, ly, lz) = rtx.DEFAULT_EYE, rtx.DEFAULT_LOOK_AT
    c, s = round(math.cos(math.radians(deg)), 12), round(math.sin(math.radians(deg)), 12)
    return (ex * c + ez * s, ey, -ex * s + ez * c), (lx * c + lz * s, ly, -lx * s + lz * c)


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
    ap.add_argument("--yardstick", default=None)
    ap.add_argument("--no-1m", action="store_true")
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
    has_rows = hasattr(scene, "render_view_rows_device")
    views = {a: rtx.Scene.view(width, height, *orbit(rtx, a)) for a in ANGLES}
    assert bytes(views[0]) == bytes(scene.own_view())
    fresh, create_ms = {}, {}
    if has_rows:
        for a in ANGLES:
            eye, look_at = orbit(rtx, a)
            t0 = time.perf_counter()
            fresh[a] = rtx.Scene(width, height, tris, rgb_in, samples, eye=eye, look_at=look_at)
            create_ms[a] = (time.perf_counter() - t0) * 1e3
    stream = torch.cuda.Stream(device="cuda:0")
    doc = {"scene": "big_bunny.obj + ground, %dx%d" % (width, height), "device": torch.cuda.get_device_name(0),
           "repeats": args.repeats, "warmup": args.warmup, "pixels": n, "orbit_eyes": {str(a): orbit(rtx, a)[0] for a in ANGLES},
           "cases": []}
    with torch.cuda.stream(stream):
        s = stream.cuda_stream
        buf = {}

        def out(name):
            buf[name] = torch.zeros(n * 3, dtype=torch.uint8, device="cuda:0")
            return buf[name].data_ptr()

        cases, expect, before = {}, {}, {}
        p = out("tiles_own")
        cases["tiles_own"] = lambda p=p: scene.render_tiles_device(0, 0, 1, height, p, n * 3, s)
        expect["tiles_own"] = 0
        if has_rows:
            p = out("view_rows_own")
            cases["view_rows_own"] = lambda p=p: scene.render_view_rows_device(0, views[0], p, n * 3, s)
            before["view_rows_own"] = cases["view_rows_own"]
            expect["view_rows_own"] = 0
        for a in ANGLES:
            if has_rows:
                p = out("view_rows_eye%d" % a)
                cases["view_rows_eye%d" % a] = lambda p=p, a=a: scene.render_view_rows_device(0, views[a], p, n * 3, s)
                expect["view_rows_eye%d" % a] = a
            p = out("view_eye%d" % a)
            cases["view_eye%d" % a] = lambda p=p, a=a: scene.render_view_device(0, views[a], p, None, None, s)
            expect["view_eye%d" % a] = a
            if has_rows:
                p = out("tiles_fresh_eye%d" % a)
                cases["tiles_fresh_eye%d" % a] = lambda p=p, a=a: fresh[a].render_tiles_device(0, 0, 1, height, p, n * 3, s)
                expect["tiles_fresh_eye%d" % a] = a
        ms = {k: [] for k in cases}
        passes = {k: [] for k in cases if k.startswith("view_rows_eye")}
        for i in range(args.warmup + args.repeats):
            for name, launch in cases.items():
                if name in before:
                    before[name]()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                launch()
                e1.record(stream)
                e1.synchronize()
                if i >= args.warmup:
                    ms[name].append(e0.elapsed_time(e1))
                    if name in passes:
                        sched, shade = scene.launch_timings(max_launches=1)
                        passes[name].append((float(sched[-1]), float(shade[-1])))
        frames = {a: scene.render_view(views[a]).reshape(n, 3) for a in ANGLES}      # rtx_render_view's bytes
        same = {k: bool(np.array_equal(buf[k].cpu().numpy().reshape(n, 3), frames[expect[k]])) for k in cases}
        for name, v in ms.items():
            more = {"same_bytes_as_render_view": same[name]}
            if name in passes:
                more["schedule_ms_median"] = round(float(np.median([x[0] for x in passes[name]])), 4)
                more["shade_ms_median"] = round(float(np.median([x[1] for x in passes[name]])), 4)
            if name.startswith("tiles_fresh_eye"):
                more["host_scene_create_ms"] = round(create_ms[int(name[len("tiles_fresh_eye"):])], 1)
            doc["cases"].append(row(name, v, **more))

        # (d) the aim kernels alone: a one-row, eight-pixel view, eyes alternating minus one eye repeated
        def aim_alone(sc, what):
            tiny = [rtx.Scene.view(8, 8, *orbit(rtx, a), rect=(0, 3, 8, 1)) for a in (90, 270)]
            d = torch.zeros(64, dtype=torch.uint8, device="cuda:0")
            t = {"alternating": [], "repeated": []}
            for i in range(args.warmup + args.repeats * 4):
                for kind in t:
                    if kind == "repeated":
                        sc.render_view_rows_device(0, tiny[0], d.data_ptr(), 64, s)
                    else:
                        sc.render_view_rows_device(0, tiny[1], d.data_ptr(), 64, s)
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record(stream)
                    sc.render_view_rows_device(0, tiny[0], d.data_ptr(), 64, s)
                    e1.record(stream)
                    e1.synchronize()
                    if i >= args.warmup:
                        t[kind].append(e0.elapsed_time(e1))
            want = sc.render_view(tiny[0]).reshape(-1)
            ok = bool(np.array_equal(d.cpu().numpy()[:24], want))
            same["aim_" + what] = ok
            alt, rep = float(np.median(t["alternating"])), float(np.median(t["repeated"]))
            doc["cases"].append({"case": "aim_" + what, "n_nodes": sc.info()["n_nodes"], "depth": sc.info()["depth"],
                                 "tiny_view_aiming_median_ms": round(alt, 4), "tiny_view_aimed_median_ms": round(rep, 4),
                                 "aim_kernels_ms": round(alt - rep, 4), "same_bytes_as_render_view": ok})

        if has_rows:
            aim_alone(scene, "big_bunny")
            if not args.no_1m:
                t1, c1 = rtx.synthetic_primitives(1000000)
                t0 = time.perf_counter()
                with rtx.Scene(64, 64, t1, c1, samples, tie_rank=None, reference_tree=rtx.REFTREE_NEVER) as big:
                    doc["synthetic_1m_scene_create_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
                    aim_alone(big, "synthetic_1m")
    for r in doc["cases"]:
        print(json.dumps(r), file=sys.stderr)
    if args.yardstick:
        with open(args.yardstick) as f:
            other = json.load(f)
        doc["parent_build"] = [r for r in other["cases"] if r["case"] == "tiles_own" or r["case"].startswith("view_eye")]
        base = next(r for r in doc["parent_build"] if r["case"] == "tiles_own")["median_ms"]
        for r in doc["cases"]:
            if "median_ms" in r:
                r["ratio_to_parent_tiles_own"] = round(r["median_ms"] / base, 3)
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
