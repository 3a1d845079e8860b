"""The scheduling pass's long mode (probe_kernel: a long tile's primary rays as four 4 x 4 pixel beams, one workgroup per
tile, started first) against its ordinary mode, through rtx_debug_probe_split: 0 the scene's prediction, 1 no tile long,
2 every tile of the frame long.  Under every mode the RGB8 bytes equal the oracle's, and the tile descriptors, hit records
and pixel slots the pass leaves, and the counted statistics, are the same words.  Small frames only: the 256 x 256 one has
a predicted list of its own, on the others mode 2 is what walks the beams."""
import importlib
import os

import numpy as np
import pytest

import np_ref
from test_gpu_spheres import KAT, kat_scene
from test_host_spheres import mixed_scene

pytestmark = pytest.mark.gpu
F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = (0, 1, 2)


@pytest.fixture(scope="module")
def rtx():
    mod = importlib.import_module("ray-tracer-rust_amd")
    assert mod.device_count() >= 1, "no HIP device: the product path has no CPU fallback"
    return mod


def model(name):
    return os.path.join(ROOT, "models", name)


def pass_words(scene):
    """what the scheduling pass of the most recent launch left: the descriptors, and per tile with a job the hit words it
    wrote (compact form: the hit points, then the shared normal and colour) and its pixel slots"""
    td = scene.tile_descs()
    hits, slots = scene.probe_records()
    out = [td.tobytes()]
    for t in np.nonzero(td[:, 1])[0]:
        n = int(td[t, 1])
        if td[t, 2] & 8:
            out.append(hits[t, :3 * n].tobytes() + hits[t, 192:198].tobytes())
        else:
            out.append(hits[t, :12 * n].tobytes())
        out.append(slots[t].tobytes())
    return out


def counted(st):
    return {k: v for k, v in st.items() if k not in ("kernel_ms", "total_ms")}


def same_under_every_mode(scene, render, ref, long_groups):
    """render() -> (image, statistics) once per mode; long_groups: mode -> the long-list workgroups the launch must have
    been handed (None: at least one).  -> the images' common bytes"""
    seen = {}
    for mode in MODES:
        scene.debug_probe_split(mode)
        img, st = render(True)
        handed = scene.debug_probe_split(mode)
        plain, _ = render(False)
        assert np.array_equal(plain, img), "mode %d: the counted and the uncounted form differ" % mode
        if long_groups[mode] is None:
            assert handed >= 1, "mode %d: no tile was long" % mode
        else:
            assert handed == long_groups[mode], "mode %d: %d long workgroups" % (mode, handed)
        seen[mode] = (img, counted(st), pass_words(scene))
    scene.debug_probe_split(0)
    for mode in MODES:
        img, st, words = seen[mode]
        diff = int((img != ref).any(axis=2).sum())
        assert diff == 0, "mode %d: %d pixels differ from the oracle" % (mode, diff)
        assert st == seen[1][1], "mode %d: statistics %s, mode 1 %s" % (mode, st, seen[1][1])
        assert len(words) == len(seen[1][2]) and all(a == b for a, b in zip(words, seen[1][2])), \
            "mode %d: the scheduling pass left other descriptors, hit records or pixel slots" % mode
    return seen[1][0]


def rows_of(scene, row0=0, nrows=None):
    return lambda stats: scene.render_rows(row0, nrows, stats=True) if stats else (scene.render_rows(row0, nrows), None)


def frame_tiles(W, H):
    return ((W + 7) // 8) * ((H + 7) // 8)


@pytest.fixture(scope="module")
def bunny64(rtx, orc, samples_seeded):
    ref, _ = orc.default_scene(["big_bunny.obj"], 64, 64, samples_seeded).render_rows(mode=orc.MODE_BVH)
    ref.setflags(write=False)
    scene = rtx.default_scene([model("big_bunny.obj")], 64, 64, samples_seeded)
    yield scene, ref
    scene.close()


@pytest.fixture(scope="module")
def bunny256(rtx, orc, samples_seeded):
    """the frame with a predicted list of its own"""
    ref, ost = orc.default_scene(["big_bunny.obj"], 256, 256, samples_seeded).render_rows(mode=orc.MODE_BVH)
    ref.setflags(write=False)
    scene = rtx.default_scene([model("big_bunny.obj")], 256, 256, samples_seeded)
    yield scene, ref, ost
    scene.close()


def test_big_bunny_256(bunny256):
    scene, ref, ost = bunny256
    predicted = len(scene.probe_long()[0])
    assert predicted >= 8
    same_under_every_mode(scene, rows_of(scene), ref, {0: predicted, 1: 0, 2: frame_tiles(256, 256)})
    assert scene.render_rows(stats=True)[1]["primary_hits"] == ost["primary_hits"]


def test_big_bunny_ragged(rtx, orc, samples_seeded):
    """203 x 117: the tiles of the right and the lower edge have beams wholly outside the frame"""
    W, H = 203, 117
    ref, ost = orc.default_scene(["big_bunny.obj"], W, H, samples_seeded).render_rows(mode=orc.MODE_BVH)
    with rtx.default_scene([model("big_bunny.obj")], W, H, samples_seeded) as scene:
        assert len(scene.probe_long()[0]) == 0                  # (a list below eight tiles is dropped)
        same_under_every_mode(scene, rows_of(scene), ref, {0: 0, 1: 0, 2: frame_tiles(W, H)})
        assert scene.render_rows(stats=True)[1]["primary_hits"] == ost["primary_hits"]


def patch_scene(rtx, quadrants, W=64, tile=(3, 3)):
    """one small triangle per listed quadrant of `tile`, facing the eye, around the ray through the quadrant's centre;
    each at its own depth and in its own colour, nothing else in the scene"""
    eye = np.zeros(3, F)
    cam = rtx.camera_new((0.0, 0.0, 0.0), (0.0, 0.0, -1.0), (0.0, 1.0, 0.0))
    half = np.full((4096, 2), 0.5, F)
    tris, rgb = [], []
    for q in quadrants:
        cx, cy = tile[0] * 8 + 4 * (q & 1) + 1, tile[1] * 8 + 4 * (q >> 1) + 1      # the pixel whose lower right corner is the centre
        _, d = np_ref.primary_rays([cx], [cy], W, W, eye, cam, 24.0, half)
        c = d[0].astype(np.float64) * (30.0 + 4.0 * q)
        r = 0.9 * (30.0 + 4.0 * q) / 24.0                                            # under one pixel's width at that depth
        tris.append(np.concatenate([c + (-r, -r, 0.0), c + (r, -r, 0.0), c + (0.0, r, 0.0)]))
        rgb.append([1.0, 0.25 + 0.25 * q, 0.5])
    return np.array(tris, F), np.array(rgb, F), half


@pytest.mark.parametrize("quadrants", [(2,), (0, 1, 2, 3)])
def test_one_beam_alone_and_four_beams_on_four_primitives(rtx, orc, quadrants):
    W = 64
    tris, rgb, half = patch_scene(rtx, quadrants)
    kw = dict(eye=(0.0, 0.0, 0.0), look_at=(0.0, 0.0, -1.0), up=(0.0, 1.0, 0.0), distance=24.0,
              light_tri=(-2.0, 9.0, -3.0, 2.0, 9.0, -3.0, 0.0, 9.0, 1.0), nb_light_sample=8)
    ref, _, otri = orc.Scene(W, W, tris, rgb, half, **kw).render_rows(mode=orc.MODE_BVH, want_tri=True)
    hit = otri != 0xFFFFFFFF
    ys, xs = np.nonzero(hit)
    assert len(ys) and (xs // 8 == 3).all() and (ys // 8 == 3).all()          # one tile holds every hit
    beam = ((ys % 8) // 4) * 2 + (xs % 8) // 4
    assert sorted(set(beam.tolist())) == sorted(quadrants)                       # exactly the listed beams hit something
    for q in quadrants:
        assert set(otri[ys[beam == q], xs[beam == q]].tolist()) == {quadrants.index(q)}, "beam %d hits its own primitive" % q
    with rtx.Scene(W, W, tris, rgb, half, tie_rank=None, **kw) as scene:
        same_under_every_mode(scene, rows_of(scene), ref, {0: 0, 1: 0, 2: 64})
        scene.debug_probe_split(2)
        scene.render_rows()
        td = scene.tile_descs()
        assert (td[:, 1] != 0).sum() == 1 and td[:, 1].sum() == hit.sum()
        assert bool(td[td[:, 1] != 0][0, 2] & 1) == (len(quadrants) == 1)        # sample-major numbering: one surface


def test_two_primary_rays_per_pixel(rtx, orc, samples_seeded):
    ref, _ = orc.default_scene(["big_bunny.obj"], 64, 64, samples_seeded, nb_ray=2).render_rows(mode=orc.MODE_BVH)
    with rtx.default_scene([model("big_bunny.obj")], 64, 64, samples_seeded, nb_ray=2) as scene:
        same_under_every_mode(scene, rows_of(scene), ref, {0: len(scene.probe_long()[0]), 1: 0, 2: 64})


def test_sphere_scene(rtx, orc, samples_seeded):
    tris, rgb, spheres, srgb, kinds = kat_scene()
    ref, _ = orc.Scene(32, 32, tris, rgb, samples_seeded, spheres=spheres, sphere_rgb=srgb, kinds=kinds,
                       **KAT).render_rows(mode=orc.MODE_BVH)
    with rtx.Scene(32, 32, tris, rgb, samples_seeded, spheres=spheres, sphere_rgb=srgb, kinds=kinds, **KAT) as scene:
        same_under_every_mode(scene, rows_of(scene), ref, {0: 0, 1: 0, 2: 16})


def test_hard_direction_in_one_beam_queues_the_tile_once(rtx, orc):
    """A sample table of halves with exact zeros for four pixels of ONE beam: their primary directions carry a zero
    component; where it is -0.0 the direction is hard and the tile goes to the reference re-render — once, whichever
    wavefront met it."""
    W = 40
    tris, rgb, spheres, srgb, kinds = mixed_scene(np.random.default_rng(31), 220, 60)
    kw = dict(eye=(0.0, 0.0, 0.0), look_at=(0.0, 0.0, -1.0), up=(0.0, 1.0, 0.0), distance=24.0,
              light_tri=(-2.0, 9.0, -3.0, 2.0, 9.0, -3.0, 0.0, 9.0, 1.0), nb_light_sample=24)
    cam = rtx.camera_new(kw["eye"], kw["look_at"], kw["up"])
    chosen = None
    for column in (0, 1):                # zeros in s0 for pixels (20, 8..11) — beam 1 of tile (2, 1) — or in s1 for (8..11, 20)
        table = np.full((4096, 2), 0.5, F)
        px = np.array([20] * 4 if column == 0 else [8, 9, 10, 11], np.uint32)
        py = np.array([8, 9, 10, 11] if column == 0 else [20] * 4, np.uint32)
        table[(px * W + py) % len(table), column] = 0.0
        _, d = np_ref.primary_rays(px, py, W, W, np.zeros(3, F), cam, 24.0, table)
        if (np.signbit(d) & (d == 0.0)).any():
            chosen = table
            break
    assert chosen is not None, "neither axis gives a -0.0 component"
    ref, ost = orc.Scene(W, W, tris, rgb, chosen, spheres=spheres, sphere_rgb=srgb, kinds=kinds, **kw).render_rows(mode=orc.MODE_BVH)
    with rtx.Scene(W, W, tris, rgb, chosen, spheres=spheres, sphere_rgb=srgb, kinds=kinds, **kw) as scene:
        same_under_every_mode(scene, rows_of(scene), ref, {0: 0, 1: 0, 2: 25})
        for mode in MODES:
            scene.debug_probe_split(mode)
            _, st = scene.render_rows(stats=True)
            assert st["redo_tiles"] == 1, "mode %d: %d tiles re-rendered" % (mode, st["redo_tiles"])
            assert ((scene.tile_descs()[:, 2] & 2) != 0).sum() == 1


def test_two_way_share_aligned(rtx, bunny256):
    """each share is handed the frame's predicted list and finds its own tiles on it: the listed tiles of the other
    share's rows leave, the rectangle around the listed tiles is in frame rows"""
    torch = pytest.importorskip("torch")
    scene, ref, _ = bunny256
    stream = torch.cuda.current_stream()

    def render(stats):
        frame = np.zeros((256, 256, 3), np.uint8)
        for first in (0, 1):
            nbytes = scene.tiles_bytes(first, 2, 8)
            buf = torch.zeros(nbytes, dtype=torch.uint8, device="cuda:0")
            scene.render_tiles_device(0, first, 2, 8, buf.data_ptr(), nbytes, stream.cuda_stream, None)
            torch.cuda.synchronize()
            rtx.scatter_tiles(frame, buf.cpu().numpy(), first, 2, 8)
        return frame, {}

    predicted = len(scene.probe_long()[0])
    assert predicted >= 8
    same_under_every_mode(scene, render, ref, {0: predicted, 1: 0, 2: frame_tiles(256, 256)})


def test_unaligned_shares_run_one_wavefront_per_tile(rtx, bunny64):
    """rows that start off a tile row, and bands of four rows: the launch's tiles are not the frame's, no mode lists any"""
    scene, ref = bunny64
    same_under_every_mode(scene, rows_of(scene, 4, 40), ref[4:44], {0: 0, 1: 0, 2: 0})
    frames = lambda stats: scene.render_frame((0, 0), 4, stats=True) if stats else (scene.render_frame((0, 0), 4), None)
    same_under_every_mode(scene, frames, ref, {0: 0, 1: 0, 2: 0})


def test_posed_scene_and_view_calls_run_one_wavefront_per_tile(rtx, bunny64, samples_seeded):
    """(a scene of its own: the pose stays with the scene)"""
    _, ref = bunny64
    with rtx.default_scene([model("big_bunny.obj")], 64, 64, samples_seeded) as scene:
        posed_and_view_calls(scene, ref)


def posed_and_view_calls(scene, ref):
    scene.pose(scene.tris)
    view = scene.own_view()
    posed = lambda stats: scene.render_view_rows(view, stats=True, posed=True) if stats else (scene.render_view_rows(view, posed=True), None)
    same_under_every_mode(scene, posed, ref, {0: 0, 1: 0, 2: 0})
    plain = lambda stats: scene.render_view_rows(view, stats=True) if stats else (scene.render_view_rows(view), None)
    same_under_every_mode(scene, plain, ref, {0: 0, 1: 0, 2: 0})
