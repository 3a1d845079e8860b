"""shade_tiles_kernel gives a job's ray loops an issue priority that depends on the job (csrc/rtx_pass_order.hpp:
kRaisedShare, and rtx_pass_shade.hpp: set_wave_priority) — which jobs run raised depends on who claims what and on the launch's order; the bytes and the
counted statistics must not.  The shapes are the smallest that reach every level and every way a job gets its level:
more jobs than workgroups (first and later jobs, costly and open-ground tiles), fewer jobs than workgroups (parts of
tiles are the jobs), the whole-stream form with its per-XCD claims, the counted form, and a second primary ray whose
pass takes its levels from a fresh order."""
import importlib
import os

import numpy as np
import pytest

import gpu_forms as gf

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUNNY = os.path.join(ROOT, "models", "big_bunny.obj")
FRAME = (512, 384)                 # 64 x 48 = 3,072 tiles: three times the 1,024 resident workgroups
BANDS = [2 * b for b in (3, 35, 67, 99, 131, 163)]          # six 2-row bands spread over the 384 rows
SHARE = dict(first_tile=3, tile_stride=8, tile_rows=8)      # rows 24..31, 88..95, ...: 6 x 64 = 384 tiles


@pytest.fixture(scope="module")
def rtx():
    mod = importlib.import_module("ray-tracer-rust_amd")
    assert mod.device_count() >= 1, "no HIP device: the product path has no CPU fallback"
    return mod


@pytest.fixture(scope="module")
def frame_scene(rtx, samples_seeded):
    with rtx.default_scene([BUNNY], FRAME[0], FRAME[1], samples_seeded) as s:
        yield s


@pytest.fixture(scope="module")
def whole_frame(frame_scene):
    """The 512 x 384 frame, rendered once and shared (read-only) by the tests that compare with it."""
    img = frame_scene.render_rows()
    img.setflags(write=False)
    return img


def same_bytes(img, ref, what):
    assert img.shape == ref.shape, what
    bad = (img != ref).any(axis=2)
    print("%s: %d of %d pixels differ" % (what, int(bad.sum()), bad.size))
    ys, xs = np.nonzero(bad)
    assert not bad.any(), "%s: %d pixels differ; first (x, y): %s" % (what, int(bad.sum()), list(zip(xs[:8].tolist(), ys[:8].tolist())))


def test_more_jobs_than_workgroups_matches_the_oracle(whole_frame, orc, samples_seeded):
    W, H = FRAME
    osc = orc.default_scene(["big_bunny.obj"], W, H, samples_seeded)
    kinds = set()
    for row0 in BANDS:
        ref, ost = osc.render_rows(row0, 2, mode=orc.MODE_BVH)
        kinds.add("hits" if ost["primary_hits"] else "sky")
        same_bytes(whole_frame[row0:row0 + 2], ref, "rows %d..%d against the oracle" % (row0, row0 + 1))
    osc.close()
    assert "hits" in kinds


def test_more_jobs_than_workgroups_is_the_same_frame_every_time(frame_scene, whole_frame):
    for k in range(3):
        same_bytes(frame_scene.render_rows(), whole_frame, "launch %d against the first" % (k + 2))


def test_fewer_jobs_than_workgroups_matches_the_whole_frame(rtx, frame_scene, whole_frame):
    torch = pytest.importorskip("torch")
    W, H = FRAME
    first, stride, rows = SHARE["first_tile"], SHARE["tile_stride"], SHARE["tile_rows"]
    nbytes = frame_scene.tiles_bytes(first, stride, rows)
    assert nbytes == rtx.tiles_rows_of(H, first, stride, rows) * W * 3
    buf = torch.full((nbytes,), 0x5A, dtype=torch.uint8, device="cuda:0")
    frame_scene.render_tiles_device(0, first, stride, rows, buf.data_ptr(), nbytes, torch.cuda.current_stream().cuda_stream, None)
    torch.cuda.synchronize()
    packed = buf.cpu().numpy().reshape(-1, W, 3)
    want = np.concatenate([whole_frame[t * rows:(t + 1) * rows] for t in range(first, (H + rows - 1) // rows, stride)])
    same_bytes(packed, want, "share %d of %d against the same rows of the whole frame" % (first, stride))


def test_whole_stream_form_matches_the_oracle(rtx, orc, samples_seeded):
    """The synthetic 100k-triangle mesh at 128 x 128 (more stream records than a tile's cut may refer to: every chunk
    walks the whole stream, jobs are claimed per XCD) against the oracle's leaf-gated brute force on the 16 x 16 centre
    crop, as bench.py checks its 1M-triangle workload."""
    W = H = 128
    side = 16
    x0, y0 = W // 2 - side // 2, H // 2 - side // 2
    tris, rgb = rtx.synthetic_primitives(100000)
    osc = orc.Scene(W, H, tris, rgb, samples_seeded, build_bvh=False)
    ref, ost = osc.render_window(x0, y0, side, side, mode=orc.MODE_LEAFBOX)
    osc.close()
    assert ost["nonfinite_t"] == 0 and ost["primary_hits"] > 0
    with rtx.Scene(W, H, tris, rgb, samples_seeded) as s:
        assert s.info()["n_nodes"] > gf.CUT_MAX_NODES, "the scene does not reach the whole-stream form"
        img, st = gf.render_both(s)
    assert st["redo_tiles"] == 0
    same_bytes(img[y0:y0 + side, x0:x0 + side], ref, "whole stream, centre crop")


def test_counted_statistics_do_not_depend_on_the_levels(frame_scene):
    stats = []
    for _ in range(2):
        _, st = frame_scene.render_rows(stats=True)
        stats.append({k: v for k, v in st.items() if isinstance(v, (int, np.integer))})
    print(stats[0])
    assert stats[0]["box_tests"] > 0 and stats[0]["wave_tri_visits"] > 0
    assert stats[0] == stats[1]


def test_two_primary_rays_match_the_oracle(rtx, orc, samples_seeded):
    W, H = 128, 96
    tris, rgb = orc.default_primitives(["big_bunny.obj"])
    osc = orc.Scene(W, H, tris, rgb, samples_seeded, nb_ray=2)
    with rtx.Scene(W, H, tris, rgb, samples_seeded, nb_ray=2) as s:
        img, st = gf.render_both(s)
    assert st["primary_rays"] == 2 * W * H
    hits = 0
    for row0 in (40, 64):          # through the bunny and its shadow; the ground in front of it
        ref, ost = osc.render_rows(row0, 2, mode=orc.MODE_BVH)
        hits += ost["primary_hits"]
        same_bytes(img[row0:row0 + 2], ref, "nb_ray 2, rows %d..%d" % (row0, row0 + 1))
    osc.close()
    assert hits > 0
