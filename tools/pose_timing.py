#!/usr/bin/env python3
"""Times posing on big_bunny's own 1920x1080 view: rtx_scene_pose_device and rtx_render_view_posed_device beside the way to
the same frame that needs no pose, a fresh scene per pose.

    pose_kernels           rtx_scene_pose_device alone on big_bunny + ground (4,969 records): the three pose kernels
    pose_kernels_1M        the same on the 1M-triangle soup + ground (--no-1m skips it)
    view_unposed           rtx_render_view_device, d_rgb only
    view_posed_identity    rtx_render_view_posed_device after the identity pose: the same frame through the pose's buffers
    posed_turn_K           the mesh turned by K of four angles about the vertical through its box centre:
                           rtx_scene_pose_device + rtx_render_view_posed_device, one event pair around both
    posed_view_turn_K      the posed view alone, the pose standing: the cost of walking the REFITTED tree
    fresh_turn_K           the same frame the old way: rtx_scene_create with the turned vertices + rtx_scene_upload (host wall
                           time, create_upload_ms) and rtx_render_view_device on the new scene (device time): a REBUILT tree

Device time between two events on the launch's stream, uncounted kernel forms.  The cases are interleaved: --repeats rounds
of one launch each after --warmup rounds; reported are the minimum, the median and the spread (max - min) / min.
view_posed_identity must give view_unposed's bytes and every posed_turn_K its fresh scene's, which the tool checks.
One JSON document on stdout, and in --out when given.

    python tools/pose_timing.py --out profiles/pose_timing.json
"""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TURN_DEGREES = (25.0, 115.0, 205.0, 295.0)


def turned(tris, n_mesh, degrees):
    """the first n_mesh triangles turned about the vertical through their box centre, float32"""
    out = np.array(tris, np.float64).reshape(-1, 3, 3)
    mesh = out[:n_mesh]
    c = 0.5 * (mesh.reshape(-1, 3).min(axis=0) + mesh.reshape(-1, 3).max(axis=0))
    a = np.deg2rad(degrees)
    x, z = mesh[..., 0] - c[0], mesh[..., 2] - c[2]
    mesh[..., 0], mesh[..., 2] = c[0] + np.cos(a) * x + np.sin(a) * z, c[2] - np.sin(a) * x + np.cos(a) * z
    return np.ascontiguousarray(out.reshape(-1, 9).astype(np.float32))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--no-1m", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch  # before librtx.so: one HIP runtime per process (tests/conftest.py)
    sys.path.insert(0, ROOT)
    rtx = importlib.import_module("ray-tracer-rust_amd")
    if rtx.device_count() < 1 or not torch.cuda.is_available():
        raise SystemExit("no HIP device: rendering has no CPU fallback")
    width, height = rtx.DEFAULT_WIDTH, rtx.DEFAULT_HEIGHT
    samples = rtx.gen_samples()
    tris, rgb_of = rtx.default_primitives([os.path.join(ROOT, "models", "big_bunny.obj")])
    n_mesh = len(tris) - 1
    scene = rtx.Scene(width, height, tris, rgb_of, samples)
    n = width * height
    poses = [turned(tris, n_mesh, d) for d in TURN_DEGREES]
    assert all(np.abs(p).max() <= scene.pose_bound() for p in poses)
    stream = torch.cuda.Stream(device="cuda:0")
    with torch.cuda.stream(stream):
        s = stream.cuda_stream
        own = scene.own_view()
        buf = {}

        def out(name):
            buf[name] = torch.zeros(n * 3, dtype=torch.uint8, device="cuda:0")
            return buf[name].data_ptr()

        d_identity = torch.from_numpy(np.ascontiguousarray(tris)).to("cuda:0")
        d_poses = [torch.from_numpy(p).to("cuda:0") for p in poses]
        stream.synchronize()

        def timed(launch):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            launch()
            e1.record(stream)
            e1.synchronize()
            return e0.elapsed_time(e1)

        def posed_view(d_pose, p):
            scene.pose_device(0, d_pose.data_ptr(), None, s)
            scene.render_view_device(0, own, p, None, None, s, posed=True)

        def identity_view(p):
            scene.render_view_device(0, own, p, None, None, s, posed=True)

        names = ["pose_kernels", "view_unposed", "view_posed_identity"]
        names += ["posed_turn_%d" % k for k in range(4)] + ["posed_view_turn_%d" % k for k in range(4)] + ["fresh_turn_%d" % k for k in range(4)]
        ms = {k: [] for k in names}
        create_ms = {k: [] for k in range(4)}
        for name in ("view_unposed", "view_posed_identity"):
            out(name)
        for k in range(4):
            out("posed_turn_%d" % k)
            out("posed_view_turn_%d" % k)
            out("fresh_turn_%d" % k)
        for i in range(args.warmup + args.repeats):
            keep = i >= args.warmup
            t = timed(lambda: scene.pose_device(0, d_identity.data_ptr(), None, s))
            ms["pose_kernels"] += [t] if keep else []
            t = timed(lambda: scene.render_view_device(0, own, buf["view_unposed"].data_ptr(), None, None, s))
            ms["view_unposed"] += [t] if keep else []
            t = timed(lambda: identity_view(buf["view_posed_identity"].data_ptr()))
            ms["view_posed_identity"] += [t] if keep else []
            for k in range(4):
                t = timed(lambda: posed_view(d_poses[k], buf["posed_turn_%d" % k].data_ptr()))
                ms["posed_turn_%d" % k] += [t] if keep else []
                t = timed(lambda: identity_view(buf["posed_view_turn_%d" % k].data_ptr()))       # the pose of turn k stands
                ms["posed_view_turn_%d" % k] += [t] if keep else []
                name = "fresh_turn_%d" % k
                t0 = time.perf_counter()
                fresh = rtx.Scene(width, height, poses[k], rgb_of, samples)
                fresh.upload(0)
                t1 = time.perf_counter()
                fresh.render_view_device(0, own, buf[name].data_ptr(), None, None, s)      # (first launch on a new scene)
                stream.synchronize()
                t = timed(lambda: fresh.render_view_device(0, own, buf[name].data_ptr(), None, None, s))
                fresh.close()
                if keep:
                    ms[name].append(t)
                    create_ms[k].append((t1 - t0) * 1e3)
        frame = buf["view_unposed"].cpu().numpy()
        same = {"pose_kernels": True, "view_unposed": True,
                "view_posed_identity": bool(np.array_equal(buf["view_posed_identity"].cpu().numpy(), frame))}
        for k in range(4):
            fresh = buf["fresh_turn_%d" % k].cpu().numpy()
            same["fresh_turn_%d" % k] = bool((fresh != frame).any())                        # another pose: another frame
            same["posed_turn_%d" % k] = bool(np.array_equal(buf["posed_turn_%d" % k].cpu().numpy(), fresh))
            same["posed_view_turn_%d" % k] = bool(np.array_equal(buf["posed_view_turn_%d" % k].cpu().numpy(), fresh))
        big = None
        if not args.no_1m:
            t0 = time.perf_counter()
            bt, brgb = rtx.synthetic_primitives(1000000)
            soup = rtx.Scene(width, height, bt, brgb, samples, reference_tree=rtx.REFTREE_NEVER, tie_rank=None)
            soup.upload(0)
            t1 = time.perf_counter()
            d_big = torch.from_numpy(np.ascontiguousarray(bt)).to("cuda:0")
            stream.synchronize()
            v = [timed(lambda: soup.pose_device(0, d_big.data_ptr(), None, s)) for _ in range(args.warmup + args.repeats)][args.warmup:]
            info = soup.info()
            big = {"case": "pose_kernels_1M", "min_ms": round(min(v), 4), "median_ms": round(float(np.median(v)), 4),
                   "spread": round((max(v) - min(v)) / min(v), 4), "records": info["n_tris"], "nodes": info["n_nodes"],
                   "depth": info["depth"], "create_upload_ms": round((t1 - t0) * 1e3, 1)}
            soup.close()
    doc = {"scene": "big_bunny.obj + ground, %dx%d, default camera, rgb only" % (width, height), "device": torch.cuda.get_device_name(0),
           "repeats": args.repeats, "warmup": args.warmup, "pixels": n, "turn_degrees": list(TURN_DEGREES), "cases": []}
    for name, v in ms.items():
        row = {"case": name, "min_ms": round(min(v), 4), "median_ms": round(float(np.median(v)), 4),
               "spread": round((max(v) - min(v)) / min(v), 4), "bytes_as_expected": same[name]}
        if name.startswith("fresh_turn_"):
            c = create_ms[int(name.rsplit("_", 1)[1])]
            row["create_upload_ms"] = {"min": round(min(c), 2), "median": round(float(np.median(c)), 2)}
        doc["cases"].append(row)
        print("%-22s min %9.4f ms  median %9.4f ms  spread %.3f  bytes as expected: %s" %
              (name, row["min_ms"], row["median_ms"], row["spread"], same[name]), file=sys.stderr)
    if big:
        doc["cases"].append(big)
        print("%-22s min %9.4f ms  median %9.4f ms  spread %.3f" % (big["case"], big["min_ms"], big["median_ms"], big["spread"]), file=sys.stderr)
    by = {r["case"]: r for r in doc["cases"]}
    doc["turns"] = []
    for k in range(4):
        posed, fresh, walk = by["posed_turn_%d" % k], by["fresh_turn_%d" % k], by["posed_view_turn_%d" % k]
        fresh_total = fresh["create_upload_ms"]["median"] + fresh["median_ms"]
        doc["turns"].append({"degrees": TURN_DEGREES[k], "pose_and_posed_view_ms": posed["median_ms"],
                             "fresh_create_upload_and_view_ms": round(fresh_total, 3),
                             "posed_is_sooner": bool(posed["median_ms"] < fresh_total),
                             "refitted_over_rebuilt_view": round(walk["median_ms"] / fresh["median_ms"], 4)})
    identity, plain = by["view_posed_identity"], by["view_unposed"]
    noise = max(identity["spread"] * identity["min_ms"], plain["spread"] * plain["min_ms"])
    doc["identity"] = {"what": "view_posed_identity median - view_unposed median against the run-to-run spread observed",
                       "excess_ms": round(identity["median_ms"] - plain["median_ms"], 4), "spread_observed_ms": round(noise, 4),
                       "within_spread": bool(identity["median_ms"] - plain["median_ms"] <= noise)}
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
