"""Scenes, launch sequences and their oracle answers for the tests of state that survives from one launch to the next
(tests/test_sequence_sets.py states, without a GPU, what the sequences can detect; tests/test_gpu_sequences.py runs them).
Plain numpy: the oracle binding (`orc`) is handed in, and for scene Wh the product binding (`rtx`) for its host-side mesh
generator; nothing here touches a device.

The library keeps grow-only buffers per scene and device (csrc/rtx_api.cpp, DeviceState): the output buffer, the queue of
tiles for the reference walk, the tile descriptors, cuts, running sums and cost buckets.  Each scene is chosen for what it
leaves there:
    P    the lattice soup of test_gpu_pipeline.soup(41), all-zero sample table, axis camera, 40 x 40, nb_ray = 3,
         nb_light_sample = 5: running sums in HBM (nb_ray > 1) and tiles queued for the reference walk
    S    test_host_spheres.mixed_scene: 150 triangles, 40 spheres, 32 x 32, nb_ray = 2, nb_light_sample = 10, seeded table
    G    floor_scene(1): one global triangle, 56 x 56, nb_light_sample = 150: two light batches, another LDS size
    B    big_bunny.obj + ground at 203 x 117, the frame of the ragged golden
    Wh   gpu_forms.whole_stream_scene: one primitive per leaf, more records than CUT_MAX_NODES: the whole-stream form
         (`whole` is part of the key of launch_probe's cached grid), 24 x 24, nb_light_sample = 4

Which ranges of P queue tiles.  A tile is queued when one of its primary rays has a -0.0 direction component
(rtx_traverse.hpp, direction_is_hard; a +0.0 component is walked by the library's own tree).  With the axis camera and the
zero table every ray of the centre column has a zero x component and every ray of the centre row a zero y component; the
column's are all +0.0, the row's are -0.0 in its left half (20 pixels x 3 rays: three tiles).  So the ranges of P's
sequence that hold row 20 queue tiles — the whole frame, (5, 35) and (8, 16) — and the others — (0, 8), (13, 3) and the
single row — queue none.  queue_free(reference, row0, nrows) says which is which from the directions themselves, and
tests/test_sequence_sets.py asserts this paragraph.

The single-row launch is the frame's last row, except on P, whose last row is empty sky in the oracle (no hit: a launch
that wrote nothing could not be told from it): there it is row 37, the last one that is not."""
import os

import numpy as np

import gpu_forms as gf

F = np.float32
NO_HIT = 0xFFFFFFFF
SEQUENCE_SCENES = ("P", "S", "G", "B")           # one scene, many launches
LIVE_SCENES = ("P", "S", "G", "Wh")              # several live scenes on one device
S_SEED = 46                                      # (seed 44, test_gpu_pipeline's, puts no sphere into the last row)
ASYNC_SPLIT, ASYNC_TILE_ROWS = 3, 5              # the device-resident shares: a 3-way split of row tiles of 5 rows


def floor_scene(seed):
    """A big tilted floor (a global triangle) with a soup hovering 0.3 .. 3 units over it, seen from above; the light
    is below the floor (shadow rays cross it at t around 1: the `t < 1.0` rule of bvh.rs:64 decides), near the horizon
    (grazing rays over the floor) or overhead."""
    rng = np.random.default_rng(seed)
    tilt = rng.uniform(-0.15, 0.15, size=2)
    def height(x, z):
        return tilt[0] * x + tilt[1] * z
    corners = np.array([[-150.0, -120.0], [160.0, -110.0], [5.0, 170.0]]) + rng.uniform(-5, 5, size=(3, 2))
    floor = np.array([[cx, height(cx, cz), cz] for cx, cz in corners], F).reshape(1, 9)
    n = 90
    c = rng.uniform(-10, 10, size=(n, 2))
    lift = rng.choice([0.3, 0.6, 0.9, 1.0, 1.1, 1.5, 3.0], size=n) * rng.uniform(0.97, 1.03, size=n)
    centre = np.stack([c[:, 0], height(c[:, 0], c[:, 1]) + lift, c[:, 1]], axis=1)
    soup = (centre[:, None, :] + rng.uniform(-0.8, 0.8, size=(n, 3, 3)) * np.array([1.0, 0.15, 1.0])).astype(F)
    e1, e2 = soup[:, 1] - soup[:, 0], soup[:, 2] - soup[:, 0]
    soup = soup[np.linalg.norm(np.cross(e1, e2), axis=1) > 1e-3].reshape(-1, 9)
    tris = np.concatenate([soup, floor]).astype(F)
    rgb = rng.uniform(0.2, 1.0, size=(len(tris), 3)).astype(F)
    where = seed % 3
    ly = (-25.0, 1.2, 40.0)[where]
    lx = (3.0, 60.0, -4.0)[where]
    light = (lx - 2.0, ly, -3.0, lx + 2.0, ly, -3.0, lx, ly + (0.5 if where == 1 else 0.0), 2.0)
    cam = dict(eye=(1.0, 30.0, 22.0), look_at=(0.0, 0.0, 0.0), up=(0.0, 1.0, 0.0), distance=70.0, light_tri=light)
    return tris, rgb, cam


# ------------------------------------------------------------------------------------------------------ the scenes
def description(name, orc, samples, rtx=None):
    """-> dict(W, H, args = (tris, rgb, table), kw = keywords both bindings take, lib_kw / orc_kw = what only rtx.Scene /
    orc.Scene takes, mode = the oracle's traversal, nb_ray, nb_light)"""
    lib_kw, orc_kw, mode, single = {}, {}, orc.MODE_BVH, None
    if name == "P":
        from test_gpu_pipeline import AXIS, soup
        tris, rgb = soup(41)
        W, H, T, kw = 40, 40, np.zeros((4096, 2), F), dict(AXIS, nb_ray=3, nb_light_sample=5)
        single = 37
    elif name == "S":
        from test_gpu_pipeline import AXIS
        from test_host_spheres import mixed_scene
        tris, rgb, spheres, srgb, kinds = mixed_scene(np.random.default_rng(S_SEED), 150, 40)
        W, H, T = 32, 32, samples
        kw = dict(AXIS, nb_ray=2, nb_light_sample=10, spheres=spheres, sphere_rgb=srgb, kinds=kinds)
    elif name == "G":
        tris, rgb, cam = floor_scene(1)
        W, H, T, kw = 56, 56, samples, dict(cam, nb_light_sample=150)
    elif name == "B":
        tris, rgb = orc.default_primitives(["big_bunny.obj"])
        W, H, T = 203, 117, samples
        kw = dict(eye=orc.EYE, look_at=orc.LOOK_AT, up=orc.UP, distance=orc.DISTANCE, light_tri=orc.LIGHT_TRI,
                  nb_ray=orc.NB_RAY, nb_light_sample=orc.NB_LIGHT_SAMPLE)
    elif name == "Wh":
        tris, rgb, extra = gf.whole_stream_scene(rtx)
        assert not extra
        W, H, T = 24, 24, samples
        kw = dict(eye=orc.EYE, look_at=orc.LOOK_AT, up=orc.UP, distance=orc.DISTANCE, light_tri=orc.LIGHT_TRI,
                  nb_ray=1, nb_light_sample=4)
        lib_kw = dict(leaf_max=1, reference_tree=rtx.REFTREE_NEVER, tie_rank=None)
        orc_kw, mode = dict(build_bvh=False), orc.MODE_LEAFBOX
    else:
        raise KeyError(name)
    return dict(name=name, W=W, H=H, args=(tris, rgb, T), kw=kw, lib_kw=lib_kw, orc_kw=orc_kw, mode=mode,
                nb_ray=kw.get("nb_ray", 1), nb_light=kw["nb_light_sample"], single=H - 1 if single is None else single)


def make_scene(rtx, d):
    return rtx.Scene(d["W"], d["H"], *d["args"], **d["kw"], **d["lib_kw"])


_built = {}


def reference(name, orc, samples, rtx=None):
    """The oracle's frame of a scene, once per process, with the primary hits of every row, so that a row range's
    expected bytes are a slice and its statistics a sum (nb_ray = 1: from the hit-primitive plane; else rendered row by
    row): dict(frame [H, W, 3], hits [H] primary hits per row, nonfinite, ties, zero / neg_zero [H] primary rays
    with a zero / a -0.0 direction component per row, desc)"""
    if name in _built:
        return _built[name]
    import shade_sets
    d = description(name, orc, samples, rtx)
    W, H = d["W"], d["H"]
    threads = min(16, os.cpu_count() or 1)
    if name == "B":
        # the frame is the oracle's, as tests/golden/make_golden.py recorded it (a fresh render costs ten seconds and
        # more); the hits per row come from the same scene without light samples, which has the same primary rays
        import json
        from PIL import Image
        gold = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
        with open(os.path.join(gold, "golden.json")) as f:
            case = json.load(f)["cases"]["ragged_bigbunny_203x117_seed"]
        assert (case["width"], case["height"], case["table"]) == (W, H, "seed")
        frame = np.asarray(Image.open(os.path.join(gold, "ragged_bigbunny_203x117_seed.png")).convert("RGB"))
        osc = orc.Scene(W, H, *d["args"], **dict(d["kw"], nb_light_sample=0))
        _, st, tri = osc.render_rows(mode=d["mode"], nthreads=threads, want_tri=True)
        hits = (tri != NO_HIT).sum(axis=1).astype(np.int64)
        assert int(hits.sum()) == st["primary_hits"] == case["primary_hits"]
        nonfinite, ties = case["nonfinite_t"] + st["nonfinite_t"], case["exact_ties"]
    elif d["nb_ray"] == 1:
        osc = orc.Scene(W, H, *d["args"], **d["kw"], **d["orc_kw"])
        frame, st, tri = osc.render_rows(mode=d["mode"], nthreads=threads, want_tri=True)
        hits = (tri != NO_HIT).sum(axis=1).astype(np.int64)
        assert int(hits.sum()) == st["primary_hits"]
        nonfinite, ties = st["nonfinite_t"], st["exact_ties"]
    else:
        osc = orc.Scene(W, H, *d["args"], **d["kw"], **d["orc_kw"])
        rows, hits, nonfinite, ties = [], np.zeros(H, np.int64), 0, 0
        for y in range(H):
            img, st = osc.render_rows(y, 1, mode=d["mode"], nthreads=threads)
            rows.append(img)
            hits[y] = st["primary_hits"]
            nonfinite += st["nonfinite_t"]
            ties += st["exact_ties"]
        frame = np.concatenate(rows)
    kw = d["kw"]
    _, raw, _, _, _ = shade_sets.camera_raw_rays(orc, W, H, kw["eye"], kw["look_at"], kw["up"], kw["distance"], d["args"][2],
                                                 d["nb_ray"])
    raw = raw.reshape(H, W * d["nb_ray"], 3)
    zero = (raw == 0).any(axis=2)
    neg_zero = ((raw == 0) & np.signbit(raw)).any(axis=2)
    frame = np.ascontiguousarray(frame)
    frame.setflags(write=False)
    _built[name] = dict(desc=d, osc=osc, frame=frame, hits=hits, nonfinite=nonfinite, ties=ties,
                        zero=zero.sum(axis=1), neg_zero=neg_zero.sum(axis=1), neg_zero_px=neg_zero.reshape(H, W, d["nb_ray"]).any(axis=2))
    return _built[name]


def queue_free(ref, row0, nrows):
    """no primary ray of the rows has a -0.0 direction component: the launch queues no tile for the reference walk"""
    return int(ref["neg_zero"][row0:row0 + nrows].sum()) == 0


def tiles_holding_a_hard_ray(ref, row0, nrows):
    """8 x 8 tiles of the launch's own grid (it starts at row0) that hold a primary ray with a -0.0 component"""
    px = ref["neg_zero_px"][row0:row0 + nrows]
    return sum(bool(px[y:y + 8, x:x + 8].any()) for y in range(0, nrows, 8) for x in range(0, px.shape[1], 8))


def launch_tiles(W, nrows):
    """(8 x 8 tiles of a launch of nrows rows, descriptors rtx_debug_tile_descs reports for it: whole 8 x 8 blocks of tiles)"""
    tx, ty = (W + 7) // 8, (nrows + 7) // 8
    return tx * ty, ((tx + 7) // 8) * ((ty + 7) // 8) * 64


def sphere_hits_in_rows(ref, orc, row0, nrows):
    """primary rays of the rows whose closest hit (orc_closest_hit) is a sphere, and all their hits"""
    import query_sets
    import shade_sets
    d = ref["desc"]
    kw, W, H = d["kw"], d["W"], d["H"]
    o, raw, _, _, _ = shade_sets.camera_raw_rays(orc, W, H, kw["eye"], kw["look_at"], kw["up"], kw["distance"], d["args"][2],
                                                 d["nb_ray"])
    pick = slice(row0 * W * d["nb_ray"], (row0 + nrows) * W * d["nb_ray"])
    exp, _ = query_sets.oracle_hits(orc, ref["osc"], o[pick], raw[pick], query_sets.HIT_DTYPE)
    hit = exp["prim"] != NO_HIT
    return int((kw["kinds"][exp["prim"][hit]] == 1).sum()), int(hit.sum())


# ------------------------------------------------------------------------------------------------------ the sequences
def launch_sequence(H, single=None):
    """(row0, nrows, counted) in order: shrinks, grows, leaves the 8-row grid, ends on the whole frame; `single` is the
    row of the one-row launch (the last row unless a scene's description names another)"""
    single = H - 1 if single is None else single
    return [(0, H, False), (0, 8, False), (13, 3, False), (0, H, True), (single, 1, False), (5, H - 5, True),
            (8, 16, False), (0, H, False)]


def full_sequence(H, single=None):
    """launch_sequence with the two rtx_render_frame calls in it: ("rows", row0, nrows, counted) / ("frame", devices,
    tile_rows).  The two-share frame stands between the whole frame and rows (0, 8), whose bytes the whole frame's
    leading bytes would otherwise already be; the one-share frame between the single row and rows (5, H-5)."""
    s = [("rows",) + x for x in launch_sequence(H, single)]
    return s[:1] + [("frame", (0, 0), 5)] + s[1:5] + [("frame", (0,), H)] + s[5:]


def share_rows(H, first_tile, stride, tile_rows):
    """frame rows of a packed share, in the order of its output buffer"""
    out = []
    for t in range(first_tile, (H + tile_rows - 1) // tile_rows, stride):
        out.extend(range(t * tile_rows, min((t + 1) * tile_rows, H)))
    return np.asarray(out, np.int64)


def step_launches(step, H):
    """the launches a step makes on the device, each as the frame rows of its output buffer"""
    if step[0] == "rows":
        return [np.arange(step[1], step[1] + step[2])]
    devices, tile_rows = step[1], step[2]
    return [share_rows(H, j, len(devices), tile_rows) for j in range(len(devices))]


def async_launches(H):
    """the back-to-back device-resident launches: (first_tile, stride) of shares 0, 1, 2, the whole frame, share 1 again"""
    return [(0, ASYNC_SPLIT), (1, ASYNC_SPLIT), (2, ASYNC_SPLIT), (0, 1), (1, ASYNC_SPLIT)]


# several live scenes: whole frames in one order, then (after S was destroyed and created again) ranges in another
LIVE_FIRST = [("P", None, False), ("S", None, False), ("Wh", None, False), ("G", None, False),
              ("S", None, True), ("P", None, True), ("Wh", None, True), ("G", None, False)]
LIVE_SECOND = [("G", (8, 16), False), ("Wh", (13, 3), False), ("S", "last", False), ("P", "from5", False), ("Wh", "from5", True),
               ("S", "from5", True), ("G", (13, 3), True), ("P", (0, 8), True), ("Wh", None, False), ("S", None, False),
               ("P", None, True), ("G", None, True)]


def live_range(H, what):
    """(row0, nrows) of an entry of LIVE_FIRST / LIVE_SECOND"""
    if what is None:
        return 0, H
    return {"last": (H - 1, 1), "from5": (5, H - 5)}[what] if isinstance(what, str) else what


def reused_buffer_differs(frame, launches):
    """Replays launches (frame rows of each output, in order) into one grow-only buffer as the library's d_out sees them.
    -> for every launch but the first, whether what it must write differs from what the buffer held there before"""
    row_bytes = frame.shape[1] * 3
    buf = np.zeros(frame.shape[0] * row_bytes, np.uint8)
    out = []
    for k, rows in enumerate(launches):
        want = frame[rows].reshape(-1)
        if k:
            out.append(not np.array_equal(buf[:len(want)], want))
        buf[:len(want)] = want
    return out
