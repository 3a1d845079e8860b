"""GPU parity tests (run with -m gpu on an MI355X).  Every render goes through the C ABI
(include/rtx.h) into the HIP kernel; the CPU oracle is only the checker.

Bar: BASELINE.json's north_star allows per-channel |delta| <= 1 LSB for the float shading (integer indexing
bit-exact).  The kernel does not evaluate powf (the byte steps are located with the host libm) and restates the
reference's f32 operations one rounding at a time, so this suite demands MORE than the north_star: every byte equal
(TOL_LSB = 0).
"""
import importlib
import json
import os

import numpy as np
import pytest
from PIL import Image

from gpu_forms import render_both

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
TOL_LSB = 0   # north_star allows 1; DESIGN.md section 2 claims exactness, so exactness is what is asserted


@pytest.fixture(scope="module")
def rtx():
    mod = importlib.import_module("ray-tracer-rust_amd")
    assert mod.device_count() >= 1, "no HIP device: the product path has no CPU fallback"
    return mod


def model(name):
    return os.path.join(ROOT, "models", name)


def golden(name):
    with open(os.path.join(GOLD, "golden.json")) as f:
        meta = json.load(f)
    return np.asarray(Image.open(os.path.join(GOLD, name + ".png")).convert("RGB")), meta["cases"][name]


def assert_image_close(img, ref, what):
    assert img.shape == ref.shape, what
    d = np.abs(img.astype(np.int32) - ref.astype(np.int32))
    nz = int((d.max(axis=2) > 0).sum())
    print("%s: max|d|=%d, pixels differing=%d of %d" % (what, d.max(), nz, d.shape[0] * d.shape[1]))
    assert d.max() <= TOL_LSB, "%s: %d px differ by more than %d LSB" % (what, int((d.max(axis=2) > TOL_LSB).sum()), TOL_LSB)
    return nz


@pytest.mark.parametrize("name", ["c1_bunny_256_seed", "c1b_bigbunny_256_seed", "c1b_bigbunny_256_half",
                                  "ragged_bigbunny_203x117_seed"])
def test_gpu_matches_golden(rtx, samples_seeded, samples_half, name):
    ref, case = golden(name)
    T = samples_seeded if case["table"] == "seed" else samples_half
    with rtx.default_scene([model(o) for o in case["objs"]], case["width"], case["height"], T) as s:
        img, st = render_both(s)
    assert st["primary_rays"] == case["width"] * case["height"]
    assert st["primary_hits"] == case["primary_hits"]          # integer: bit-exact
    assert st["rays"] == case["r_total"]
    assert_image_close(img, ref, name)


def test_gpu_brute_force_equals_bvh_and_oracle(rtx, orc, samples_seeded):
    """RTX_ACCEL_BRUTE (one leaf with every triangle) and RTX_ACCEL_BVH give the same bytes, and both
    match the oracle's faithful BVH on a 64x64 crop that has bunny, ground and shadow."""
    W = H = 64
    with rtx.default_scene([model("big_bunny.obj")], W, H, samples_seeded) as s:
        a, sa = render_both(s)
    with rtx.default_scene([model("big_bunny.obj")], W, H, samples_seeded, accel=rtx.ACCEL_BRUTE) as s:
        assert s.info()["n_nodes"] == 1
        b, sb = render_both(s)
    assert np.array_equal(a, b)
    assert sa["primary_hits"] == sb["primary_hits"] and sb["tri_tests"] >= sa["tri_tests"]
    ref, ost = orc.default_scene(["big_bunny.obj"], W, H, samples_seeded).render_rows(mode=orc.MODE_BVH)
    assert sa["primary_hits"] == ost["primary_hits"]
    assert_image_close(a, ref, "64x64 vs oracle")


def test_rows_tiles_and_frames_are_identical(rtx, samples_seeded):
    """Any partition of the frame into row ranges / interleaved tiles gives the same bytes
    (the multi-GPU determinism requirement, exercised on one device)."""
    W, H = 203, 117
    with rtx.default_scene([model("big_bunny.obj")], W, H, samples_seeded) as s:
        full = s.render_rows()
        parts = [s.render_rows(r0, n) for r0, n in ((0, 1), (1, 7), (8, 50), (58, 59))]
        assert np.array_equal(np.concatenate(parts), full)
        for tile_rows in (1, 5, 8, 16, 117, 200):
            assert np.array_equal(s.render_frame((0,), tile_rows), full), tile_rows
        # packed tile sets as a rank of a 3-rank job would render them
        for world, tile_rows in ((2, 8), (3, 5), (8, 16)):
            frame = np.zeros_like(full)
            for rank in range(world):
                rows = s.tiles_rows(rank, world, tile_rows)
                assert s.tiles_bytes(rank, world, tile_rows) == rows * W * 3
                packed = np.concatenate(
                    [full[t * tile_rows:(t + 1) * tile_rows] for t in range(rank, (H + tile_rows - 1) // tile_rows, world)]
                    or [np.zeros((0, W, 3), np.uint8)])
                assert len(packed) == rows
                rtx.scatter_tiles(frame, packed, rank, world, tile_rows)
            assert np.array_equal(frame, full)
        empty, st = s.render_rows(10, 0, stats=True)
        assert empty.shape == (0, W, 3) and st["rays"] == 0
        with pytest.raises(rtx.RtxError) as e:
            s.render_rows(100, 18)
        assert e.value.code == rtx.ERR_BAD_ARG
        with pytest.raises(rtx.RtxError) as e:
            s.render_rows(0, 1, device=99)
        assert e.value.code == rtx.ERR_NO_DEVICE


def test_render_frame_with_several_shares_on_one_device(rtx, samples_seeded):
    """rtx_render_frame's multi-share path (one share per entry of devices[]: launch everywhere, staged D2H, gather) on a
    one-GPU box: device 0 named two, three and eight times.  Bytes and the summed counters must be those of the
    one-share frame; device order in the array must not matter."""
    W, H = 203, 117
    with rtx.default_scene([model("big_bunny.obj")], W, H, samples_seeded) as s:
        full, st1 = s.render_frame((0,), 8, stats=True)
        assert np.array_equal(full, s.render_rows())
        for devices, tile_rows in (((0, 0), 8), ((0, 0, 0), 5), ((0,) * 8, 16), ((0, 0), 200)):
            img, st = s.render_frame(devices, tile_rows, stats=True)
            assert np.array_equal(img, full), (devices, tile_rows)
            for key in ("primary_rays", "primary_hits", "shadow_rays", "rays", "redo_tiles"):
                assert st[key] == st1[key], (key, devices)
            assert st["kernel_ms"] > 0.0
            assert np.array_equal(s.render_frame(devices, tile_rows), full)      # without statistics too
        with pytest.raises(rtx.RtxError) as e:
            s.render_frame((0, 99), 8)
        assert e.value.code == rtx.ERR_NO_DEVICE


def test_tile_descriptors_follow_the_documented_block_numbering(rtx, samples_seeded):
    """include/rtx.h, rtx_debug_tile_descs: tiles are numbered by 8 x 8 blocks; padding tiles hold no hit; per tile the
    hit count equals the number of non-sky pixels of the frame the same launch produced (the default scene's sky is the only
    black: every hit pixel of a ragged 203 x 117 frame is lit by at least one sample or lies on the grey ground)."""
    W, H = 203, 117
    with rtx.default_scene([model("big_bunny.obj")], W, H, samples_seeded) as s:
        img, st = s.render_rows(stats=True)
        td = s.tile_descs(0)
    tiles_x, tiles_y = (W + 7) // 8, (H + 7) // 8
    blocks_x, blocks_y = (tiles_x + 7) // 8, (tiles_y + 7) // 8
    assert len(td) == blocks_x * blocks_y * 64
    assert int(td[:, 1].sum()) == st["primary_hits"]
    seen = set()
    for t in range(len(td)):
        b, j = t >> 6, t & 63
        x, y = (b % blocks_x) * 8 + (j & 7), (b // blocks_x) * 8 + (j >> 3)
        n_hit = int(td[t, 1])
        if x >= tiles_x or y >= tiles_y:
            assert n_hit == 0 and td[t, 0] == 0xFFFFFFFF, "padding tile %d holds work" % t
            continue
        seen.add((x, y))
        patch = img[y * 8:(y + 1) * 8, x * 8:(x + 1) * 8]
        assert n_hit <= patch.shape[0] * patch.shape[1]
        if n_hit == 0:
            assert not patch.any(), "tile (%d, %d): no hit but a lit pixel" % (x, y)
        else:
            assert int((patch.max(axis=2) > 0).sum()) <= n_hit
    assert len(seen) == tiles_x * tiles_y


def test_device_resident_entry_point(rtx, samples_seeded):
    """rtx_render_tiles_device writes into caller-owned device memory on the caller's stream
    (torch tensor + torch stream: the bench.py plumbing)."""
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("torch sees no GPU")
    W, H, world, tile_rows = 203, 117, 2, 8
    with rtx.default_scene([model("big_bunny.obj")], W, H, samples_seeded) as s:
        full = s.render_rows()
        frame = np.zeros_like(full)
        for rank in range(world):
            nbytes = s.tiles_bytes(rank, world, tile_rows)
            buf = torch.zeros(nbytes, dtype=torch.uint8, device="cuda:0")
            ctr = torch.zeros(8, dtype=torch.int64, device="cuda:0")
            stream = torch.cuda.current_stream().cuda_stream
            s.render_tiles_device(0, rank, world, tile_rows, buf.data_ptr(), nbytes, stream, ctr.data_ptr())
            torch.cuda.synchronize()
            packed = buf.cpu().numpy().reshape(-1, W, 3)
            rtx.scatter_tiles(frame, packed, rank, world, tile_rows)
            assert int(ctr[0]) > 0
        assert np.array_equal(frame, full)


def test_nb_ray_two(rtx, orc, samples_seeded):
    """NB_RAY = 2: ray i uses T[(px*W+py+i) % n] and light sample T[(r*NB_RAY+i) % n] (main.rs:162,194)."""
    W = H = 48
    tris, rgb = orc.default_primitives(["big_bunny.obj"])
    ref, ost = orc.Scene(W, H, tris, rgb, samples_seeded, nb_ray=2, nb_light_sample=20).render_rows(mode=orc.MODE_BVH)
    with rtx.Scene(W, H, tris, rgb, samples_seeded, nb_ray=2, nb_light_sample=20) as s:
        img, st = render_both(s)
    assert st["primary_rays"] == 2 * W * H and st["primary_hits"] == ost["primary_hits"]
    assert st["shadow_rays"] == ost["shadow_rays"]
    assert_image_close(img, ref, "nb_ray=2")


def _facing_camera_scene(W=32, H=32):
    # camera at the origin looking down -z: u=(1,0,0), v=(0,-1,0)... image y grows downward
    return dict(eye=(0.0, 0.0, 0.0), look_at=(0.0, 0.0, -1.0), up=(0.0, 1.0, 0.0), distance=16.0,
                light_tri=(-1.0, 50.0, -1.0, 1.0, 50.0, -1.0, 0.0, 50.0, 1.0))


def test_exact_tie_returns_reference_leaf(rtx, orc, samples_seeded):
    """Coincident triangles with different colours: every hit is an exact distance tie; the reference
    returns the right-most leaf of ITS tree (bvh.rs:123-130).  GPU (with tie_rank from
    rtxh_ref_leaf_rank) must pick the same triangle as the oracle's faithful BVH."""
    W = H = 32
    big = [-30.0, -30.0, -20.0, 30.0, -30.0, -20.0, 0.0, 30.0, -20.0]
    tris = np.array([big, big, big, big, big], dtype=np.float32)
    rgb = np.array([[1, 0, 0], [0, 1, 0], [0, 0, 1], [1, 1, 0], [0, 1, 1]], dtype=np.float32)
    kw = _facing_camera_scene()
    osc = orc.Scene(W, H, tris, rgb, samples_seeded, **kw)
    ref, ost, otri = osc.render_rows(mode=orc.MODE_BVH, want_tri=True)
    assert ost["exact_ties"] > 0
    winner = int(otri[H // 2, W // 2])
    assert osc.leaf_order()[-1] == winner
    with rtx.Scene(W, H, tris, rgb, samples_seeded, **kw) as s:
        assert np.array_equal(np.argsort(rtx.ref_leaf_rank(tris)), osc.leaf_order())
        assert s.info()["n_ref_nodes"] == 2 * len(tris) - 1
        img = s.render_rows()
    assert_image_close(img, ref, "tie scene")
    lit = img[H // 2, W // 2].astype(int)
    assert (lit > 0).tolist() == (rgb[winner] > 0).tolist()


def test_hits_closer_than_one_are_ignored(rtx, orc, samples_seeded):
    """bvh.rs:64-67: a triangle nearer than t = 1.0 is invisible; the one behind it is seen."""
    W = H = 32
    near = [-3.0, -3.0, -0.5, 3.0, -3.0, -0.5, 0.0, 3.0, -0.5]       # t ~ 0.5..0.9 for every pixel
    far = [-30.0, -30.0, -20.0, 30.0, -30.0, -20.0, 0.0, 30.0, -20.0]
    tris = np.array([near, far], dtype=np.float32)
    rgb = np.array([[1, 0, 0], [0, 1, 0]], dtype=np.float32)
    kw = _facing_camera_scene()
    ref, ost, otri = orc.Scene(W, H, tris, rgb, samples_seeded, **kw).render_rows(mode=orc.MODE_BVH, want_tri=True)
    assert (otri[otri != 0xFFFFFFFF] == 1).all() and ost["primary_hits"] > 0
    with rtx.Scene(W, H, tris, rgb, samples_seeded, **kw) as s:
        img, st = render_both(s)
    assert st["primary_hits"] == ost["primary_hits"]
    assert_image_close(img, ref, "t<1 scene")
    assert img[..., 0].max() == 0        # nothing red


def test_full_size_1080p_whole_frame_against_the_oracle(rtx, orc, samples_seeded, samples_half):
    """BASELINE configs[2] (the metric's configuration) at full size, seeded table: EVERY byte of the 1920x1080 frame
    against the oracle's faithful BVH (about 30 s of oracle time on the box's cores), plus the integer counts.
    configs[1,2] with the constant table: counts equal the survey's probe numbers (pinned to the oracle in
    tests/test_oracle_numpy.py), partition invariance, sampled oracle rows."""
    W, H = 1920, 1080
    with rtx.default_scene([model("big_bunny.obj")], W, H, samples_seeded) as s:
        img2, st2 = s.render_rows(stats=True)
        assert np.array_equal(s.render_frame((0,), 16), img2)
    ref2, ost2 = orc.default_scene(["big_bunny.obj"], W, H, samples_seeded).render_rows(mode=orc.MODE_BVH)
    assert st2["primary_hits"] == ost2["primary_hits"] and st2["redo_tiles"] == 0
    assert st2["rays"] == W * H + 100 * ost2["primary_hits"]
    assert ost2["nonfinite_t"] == 0 and ost2["assert_tmin_gt_tmax"] == 0
    assert assert_image_close(img2, ref2, "1080p seeded, whole frame") == 0
    with rtx.default_scene([model("big_bunny.obj")], W, H, samples_half) as s:
        img, st = s.render_rows(stats=True)
        assert st["primary_hits"] == 37005 + 999919        # SURVEY §8(d), reproduced by the oracle in test_oracle_numpy
        assert st["rays"] == W * H + 100 * (37005 + 999919)
        assert np.array_equal(s.render_frame((0,), 16), img)
        assert not img[:427].any()                          # sky: no hit above the bunny's first row
    osc = orc.default_scene(["big_bunny.obj"], W, H, samples_half)
    for row0, n in ((500, 2), (560, 2), (664, 2), (1078, 2)):
        ref, _ = osc.render_rows(row0, n, mode=orc.MODE_BVH)
        assert_image_close(img[row0:row0 + n], ref, "1080p half rows %d" % row0)
    with rtx.default_scene([model("bunny.obj")], W, H, samples_half) as s:     # configs[1]
        img3, st3 = s.render_rows(stats=True)
    assert st3["primary_hits"] == 1022304
    ref, _ = orc.default_scene(["bunny.obj"], W, H, samples_half).render_rows(800, 2, mode=orc.MODE_BVH)
    assert_image_close(img3[800:802], ref, "bunny.obj 1080p")


def test_configs1_bunny_1080p_whole_frame_against_the_oracle(rtx, orc, samples_seeded):
    """BASELINE configs[1] at full size with the seeded table: EVERY byte of the 1920x1080 frame of bunny.obj against the
    oracle's faithful BVH.  The mesh is sub-pixel under the hard-coded camera, so the frame is the ground
    plane's soft-lit half — the open-ground path of shade_tiles_kernel on all of it — and costs the oracle ~15 s."""
    W, H = 1920, 1080
    with rtx.default_scene([model("bunny.obj")], W, H, samples_seeded) as s:
        img, st = s.render_rows(stats=True)
        assert np.array_equal(s.render_frame((0,), 8), img)
    ref, ost = orc.default_scene(["bunny.obj"], W, H, samples_seeded).render_rows(mode=orc.MODE_BVH)
    assert st["primary_hits"] == ost["primary_hits"] and st["redo_tiles"] == 0
    assert st["rays"] == W * H + 100 * ost["primary_hits"]
    assert ost["nonfinite_t"] == 0 and ost["assert_tmin_gt_tmax"] == 0
    assert assert_image_close(img, ref, "bunny.obj 1080p seeded, whole frame") == 0


def test_synthetic_1m_triangles_4096_square_full_size(rtx, orc, samples_seeded):
    """BASELINE configs[4] at ITS size: 1,000,000 random triangles + the ground (1,000,001 primitives), 4096x4096,
    through rtx_render_tiles_device (the entry point bench.py uses).
      * every tile rendered exactly once: two buffers pre-filled with different bytes come out identical;
      * integer bound: lit (non-black) pixels <= primary hits, and the hit count of an interleaved 4-way partition
        of the frame sums to the whole frame's, its bytes scatter back to the same frame (size-independent property);
      * no tile went through the reference re-render (no -0.0 direction in this configuration);
      * oracle parity where the CPU can reach: three 64-pixel row segments — through the soup's silhouette, inside
        its shadow on the ground, open ground — in leaf-gated brute-force mode (the reference's O(n^2) tree is not
        buildable at 10^6 primitives; that mode equals the faithful BVH for every ray without a -0.0 direction
        component, DESIGN.md section 2, and exact ties are asserted absent)."""
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("torch sees no GPU")
    W = H = 4096
    tris, rgb = rtx.synthetic_primitives(1000000)
    assert len(tris) == 1000001
    stream = torch.cuda.current_stream().cuda_stream
    with rtx.Scene(W, H, tris, rgb, samples_seeded) as s:
        info = s.info()
        assert info["n_tris"] == 1000001 and info["n_ref_nodes"] == 0 and info["n_global"] == 1
        nbytes = s.tiles_bytes(0, 1, 8)
        assert nbytes == W * H * 3
        ctr = torch.zeros(8, dtype=torch.int64, device="cuda:0")
        frames = []
        for filler in (0xAA, 0x55):
            buf = torch.full((nbytes,), filler, dtype=torch.uint8, device="cuda:0")
            s.render_tiles_device(0, 0, 1, 8, buf.data_ptr(), nbytes, stream, ctr.data_ptr() if filler == 0xAA else None)
            torch.cuda.synchronize()
            frames.append(buf.cpu().numpy().reshape(H, W, 3))
            del buf
        hits, redo = int(ctr[0]), int(ctr[5])
        assert np.array_equal(frames[0], frames[1])
        frame = frames[0]
        del frames
        lit = int((frame.reshape(-1, 3).max(axis=1) > 0).sum())
        assert redo == 0 and 0.5 * hits < lit <= hits
        # interleaved partition, as four ranks would render it
        world, tile_rows, part_hits = 4, 8, 0
        again = np.zeros_like(frame)
        for rank in range(world):
            nb = s.tiles_bytes(rank, world, tile_rows)
            buf = torch.full((nb,), 0x33, dtype=torch.uint8, device="cuda:0")
            c = torch.zeros(8, dtype=torch.int64, device="cuda:0")
            s.render_tiles_device(0, rank, world, tile_rows, buf.data_ptr(), nb, stream, c.data_ptr())
            torch.cuda.synchronize()
            part_hits += int(c[0])
            rtx.scatter_tiles(again, buf.cpu().numpy().reshape(-1, W, 3), rank, world, tile_rows)
            del buf
        assert part_hits == hits and np.array_equal(again, frame)
    osc = orc.Scene(W, H, tris, rgb, samples_seeded, build_bvh=False)
    # the soup fills x 1820..2280 / y 1880..2350 or so of the frame (the big_bunny box seen by the default camera)
    for col0, row in ((1790, 2100), (2048, 2480), (300, 3900)):
        ref, ost = osc.render_window(col0, row, 64, 1, mode=orc.MODE_LEAFBOX)
        assert ost["nonfinite_t"] == 0
        got = frame[row:row + 1, col0:col0 + 64]
        print("configs[4] segment x %d..%d y %d: oracle hits %d, box tests %d" % (col0, col0 + 63, row, ost["primary_hits"], ost["slab_tests"]))
        assert np.array_equal(got, ref), "segment at x=%d y=%d" % (col0, row)


def _random_soup(rng, n, lattice):
    """Triangles with vertices on an integer lattice (many exactly axis-aligned edges / flat boxes /
    shared planes) or at random float positions."""
    if lattice:
        v = rng.integers(-6, 7, size=(n, 3, 3)).astype(np.float32)
        v[..., 2] -= 14.0
    else:
        c = rng.uniform(-6, 6, size=(n, 1, 3)).astype(np.float32)
        c[..., 2] -= 14.0
        v = c + rng.uniform(-2.5, 2.5, size=(n, 3, 3)).astype(np.float32)
    e1, e2 = v[:, 1] - v[:, 0], v[:, 2] - v[:, 0]
    keep = np.linalg.norm(np.cross(e1, e2), axis=1) > 1e-3          # drop zero-area (NaN normals)
    v = v[keep]
    rgb = rng.uniform(0.2, 1.0, size=(len(v), 3)).astype(np.float32)
    return v.reshape(-1, 9), rgb


@pytest.mark.parametrize("seed,lattice,table", [(1, True, "zero"), (2, True, "zero"), (3, True, "seed"),
                                                (4, False, "seed"), (5, False, "zero"), (6, True, "half")])
def test_random_soups_including_degenerate_rays(rtx, orc, samples_seeded, samples_half, seed, lattice, table):
    """Random triangle soups seen by an axis-aligned camera at the origin.  With an all-zero sample table the
    primary directions are (px-W/2, -(py-H/2), -d)/norm: exact zeros on the centre row and column, origin
    coordinates equal to lattice box faces -> the 0/0 and +-inf corners of the slab test, and the wave-wide
    switch from the multiply-based culling to the exact test.  GPU must equal the oracle's faithful BVH."""
    rng = np.random.default_rng(seed)
    tris, rgb = _random_soup(rng, 300, lattice)
    T = {"zero": np.zeros((4096, 2), np.float32), "seed": samples_seeded, "half": samples_half}[table]
    kw = dict(eye=(0.0, 0.0, 0.0), look_at=(0.0, 0.0, -1.0), up=(0.0, 1.0, 0.0), distance=24.0,
              light_tri=(-2.0, 9.0, -3.0, 2.0, 9.0, -3.0, 0.0, 9.0, 1.0), nb_light_sample=24)
    W, H = 40, 40
    ref, ost, otri = orc.Scene(W, H, tris, rgb, T, **kw).render_rows(mode=orc.MODE_BVH, want_tri=True)
    assert ost["nonfinite_t"] == 0 and ost["primary_hits"] > 100
    with rtx.Scene(W, H, tris, rgb, T, **kw) as s:
        img, st = render_both(s)
    assert st["primary_hits"] == ost["primary_hits"]
    nz = assert_image_close(img, ref, "soup seed %d" % seed)
    assert nz == 0


def test_synthetic_soup_with_reference_tree(rtx, orc, samples_seeded):
    """BASELINE configs[4] at test size: 20,000-triangle random soup in the big_bunny AABB + ground.  Small enough for
    the reference's O(n^2) tree, so the oracle's faithful BVH is the checker and the library builds the same tree."""
    W = H = 64
    tris, rgb = rtx.synthetic_primitives(20000)
    ref, ost = orc.Scene(W, H, tris, rgb, samples_seeded, nb_light_sample=24).render_rows(mode=orc.MODE_BVH)
    with rtx.Scene(W, H, tris, rgb, samples_seeded, nb_light_sample=24) as s:
        assert s.info()["n_ref_nodes"] == 2 * len(tris) - 1
        img, st = render_both(s)
    assert st["primary_hits"] == ost["primary_hits"] and st["redo_tiles"] == 0
    assert assert_image_close(img, ref, "synthetic 20k") == 0


def test_synthetic_soup_beyond_reference_tree(rtx, orc, samples_seeded):
    """60,001 primitives: past RTX_REFTREE_AUTO's limit, no reference tree (the reference could not build one in
    reasonable time either).  Checker: the oracle's leaf-gated brute force, which equals the faithful BVH for
    every ray without a -0.0 direction component; exact ties would be the only other
    difference and are asserted absent."""
    W = H = 32
    tris, rgb = rtx.synthetic_primitives(60000)
    osc = orc.Scene(W, H, tris, rgb, samples_seeded, nb_light_sample=8, build_bvh=False)
    ref, ost = osc.render_rows(mode=orc.MODE_LEAFBOX)
    with rtx.Scene(W, H, tris, rgb, samples_seeded, nb_light_sample=8) as s:
        assert s.info()["n_ref_nodes"] == 0
        img, st = render_both(s)
    assert st["primary_hits"] == ost["primary_hits"] and st["redo_tiles"] == 0
    assert assert_image_close(img, ref, "synthetic 60k") == 0


def test_every_kernel_variant_gives_the_same_bytes(samples_seeded):
    """The kernel variants kept for ablation (exact vs multiply-based culling, 1/2/4/8 wavefronts per tile, the
    streamed three-kernel pipeline, two rays per lane with packed f32) must all reproduce the golden image.
    They live in librtx_ablation.so only (RTX_PY_ABLATION=1 makes the Python binding load it); RTX_VARIANT is read
    once per process there, so each variant renders in its own child process (one at a time).  librtx.so itself has
    one pipeline and reads no environment variable (checked on the CPU: tests/test_host_prep.py)."""
    import subprocess
    import sys
    ref, case = golden("c1b_bigbunny_256_seed")
    code = (
        "import importlib, sys, hashlib; sys.path.insert(0, %r)\n"
        "rtx = importlib.import_module('ray-tracer-rust_amd')\n"
        "s = rtx.default_scene([%r], 256, 256, rtx.gen_samples())\n"
        "img, st = s.render_rows(stats=True)\n"
        "print('RESULT', hashlib.sha1(img.tobytes()).hexdigest(), st['primary_hits'], st['rays'])\n"
    ) % (ROOT, model("big_bunny.obj"))
    import hashlib
    want = hashlib.sha1(np.ascontiguousarray(ref).tobytes()).hexdigest()
    for variant in (0, 1, 2, 3, 5, 7, 8, 9, 25, 34, 35):
        env = dict(os.environ, RTX_VARIANT=str(variant), RTX_PY_ABLATION="1")
        out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
        line = [l for l in out.stdout.splitlines() if l.startswith("RESULT")]
        assert line, (variant, out.stderr[-800:])
        _, sha, hits, rays = line[0].split()
        assert sha == want and int(hits) == case["primary_hits"] and int(rays) == case["r_total"], (variant, line[0])


def test_north_star_variants_give_the_same_bytes(samples_seeded):
    """BASELINE.json's north_star names a design — LDS-staged triangle blocks, wavefront-level min reductions for the
    closest hit, records served from LDS — that the shipped pipeline replaced by a wave-uniform walk on scalar operands.
    librtx_ablation.so carries it as three measurable modes (RTX_J1=1: the shading pass's records as vector operands out of
    an LDS window / vector loads; 2: primary rays against LDS-staged blocks of 64 primitives, ray per lane; 3: triangle
    per lane with a DPP min-reduction per ray; csrc/rtx_j1_ablation.hpp).  Each must reproduce the golden image; what
    they cost is in DESIGN.md section 4 (profiles/r03/j1_*)."""
    import hashlib
    import subprocess
    import sys
    ref, case = golden("c1b_bigbunny_256_seed")
    code = (
        "import importlib, sys, hashlib; sys.path.insert(0, %r)\n"
        "rtx = importlib.import_module('ray-tracer-rust_amd')\n"
        "s = rtx.default_scene([%r], 256, 256, rtx.gen_samples())\n"
        "img, st = s.render_rows(stats=True)\n"
        "print('RESULT', hashlib.sha1(img.tobytes()).hexdigest(), st['primary_hits'], st['rays'])\n"
    ) % (ROOT, model("big_bunny.obj"))
    want = hashlib.sha1(np.ascontiguousarray(ref).tobytes()).hexdigest()
    for mode in (1, 2, 3):
        env = dict(os.environ, RTX_J1=str(mode), RTX_PY_ABLATION="1")
        env.pop("RTX_VARIANT", None)
        out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=600)
        line = [l for l in out.stdout.splitlines() if l.startswith("RESULT")]
        assert line, (mode, out.stderr[-800:])
        _, sha, hits, rays = line[0].split()
        assert sha == want and int(hits) == case["primary_hits"] and int(rays) == case["r_total"], (mode, line[0])
