"""Scenes and helpers for the GPU tests that pin each compiled form of the kernels (tests/test_gpu_kernel_forms.py and
the edge scenes of the other GPU modules).  Plain numpy: importing this module needs no device and no library; the
binding (`rtx`) and the oracle binding (`orc`) are handed in by the caller.

librtx.so chooses probe_kernel / shade_tiles_kernel<COUNT, .., SPHERES, WHOLE> and reference_tiles_kernel<COUNT, SPHERES>
per launch (csrc/rtx_kernel.hip, launch_dispatch / launch_probe):
    COUNT    the caller asked for statistics              -> render_both() runs both
    SPHERES  the scene holds a sphere                     -> whole_stream_scene(n_spheres=...)
    WHOLE    the stream has more than CUT_MAX_NODES records -> whole_stream_scene() (one primitive per leaf)
and inside each, advance_to_leaf (csrc/rtx_traverse.hpp) runs one of nine copies of the box loop, picked from the signs
of the walking lanes' directions -> octant_scene() / general_loop_scene()."""
import numpy as np

F = np.float32
NO_HIT = 0xFFFFFFFF
CUT_MAX_NODES = 1 << 16          # rtx_device.h, kCutMaxNodes: above it every chunk walks the whole stream


def render_both(scene, row0=0, nrows=None):
    """Render with statistics (the COUNT = true compilations) and then without (COUNT = false: what bench.py times and
    what a caller without RtxStats gets); the two must be the same bytes.  -> (uncounted image, statistics)"""
    counted, stats = scene.render_rows(row0, nrows, stats=True)
    plain = scene.render_rows(row0, nrows)
    assert plain.shape == counted.shape
    differing = int((plain != counted).any(axis=2).sum())
    assert differing == 0, "the counted and the uncounted compilation differ in %d pixels" % differing
    return plain, stats


# ---------------------------------------------------------------------------------------------- whole-stream scenes
WHOLE_N = 35000                  # synthetic triangles; + the ground, one per leaf: 70,001 stream records
WHOLE_N_QUEUED = 32800           # the smallest round count above 32,769 (the reference's O(n^2) tree is built for this one)


def whole_stream_scene(rtx, n=WHOLE_N, n_spheres=0, seed=7):
    """rtx.synthetic_primitives(n) (a soup in the big_bunny box + the ground, default camera), to be created with
    leaf_max=1 so that the stream passes CUT_MAX_NODES; optionally n_spheres spheres inside the soup's box, spread
    through the primitive order.  -> (tris, rgb, extra) where extra holds spheres / sphere_rgb / kinds or is empty."""
    tris, rgb = rtx.synthetic_primitives(n)
    if not n_spheres:
        return tris, rgb, {}
    rng = np.random.default_rng(seed)
    v = tris[:-1].reshape(-1, 3)                                  # the soup without the ground
    lo, hi = v.min(axis=0), v.max(axis=0)
    span = hi - lo
    centres = rng.uniform(lo + 0.1 * span, hi - 0.1 * span, size=(n_spheres, 3))
    radius = rng.uniform(0.008, 0.03, size=(n_spheres, 1)) * float(span.max())
    spheres = np.concatenate([centres, radius], axis=1).astype(F)
    srgb = rng.uniform(0.2, 1.0, size=(n_spheres, 3)).astype(F)
    kinds = np.zeros(len(tris) + n_spheres, np.uint8)
    kinds[np.linspace(0, len(kinds) - 2, n_spheres).astype(np.int64)] = 1      # interleaved; the ground stays last
    return tris, rgb, dict(spheres=spheres, sphere_rgb=srgb, kinds=kinds)


AXIS_CAMERA = dict(eye=(0.0, 0.0, 0.0), look_at=(0.0, 0.0, -1.0), up=(0.0, 1.0, 0.0), distance=24.0,
                   light_tri=(-2.0, 9.0, -3.0, 2.0, 9.0, -3.0, 0.0, 9.0, 1.0))


def into_axis_view(tris, extra):
    """Translate and scale a primitive list (the ground and the spheres included: the count does not change) so that
    the soup — every triangle but the last, the ground — fills x, y in -6..6 and z in -20..-8: the view of AXIS_CAMERA.
    -> (tris, extra)"""
    v = tris.reshape(-1, 3, 3).astype(np.float64)
    soup = v[:-1].reshape(-1, 3)
    lo, hi = soup.min(axis=0), soup.max(axis=0)
    scale = 12.0 / float((hi - lo).max())
    shift = np.array([0.0, 0.0, -14.0])
    out = (v - 0.5 * (lo + hi)) * scale + shift
    if extra:
        s = extra["spheres"].astype(np.float64)
        moved = np.concatenate([(s[:, :3] - 0.5 * (lo + hi)) * scale + shift, s[:, 3:] * scale], axis=1)
        extra = dict(extra, spheres=np.ascontiguousarray(moved.astype(F)))
    return np.ascontiguousarray(out.astype(F).reshape(-1, 9)), extra


# ---------------------------------------------------------------------------------------------- octant scenes
OCT_CENTRE = np.array([3.0, -2.0, 5.0])
OCT_EXTENT = 20.0
OCT_FRAME = (64, 48)
OCT_LIGHT_SAMPLES = 24
OCT_DISTANCE = 150.0             # narrow field of view: 32 u + 24 v stays far below 150 w on every axis
OCT_EYE_OFFSET = 58.0            # per axis: the eye sits on the soup's diagonal, outside its box
OCT_LIGHT_OFFSET = 45.0          # per axis, to the light triangle's centre


def octant_signs(k):
    """+1 / -1 per axis for octant k in the sense of walk_octant: bit a set = direction component a negative."""
    return np.array([-1.0 if (k >> a) & 1 else 1.0 for a in range(3)])


def octant_soup(seed, n=2000, size=2.2, n_spheres=0):
    """A compact soup of n triangles centred at OCT_CENTRE within OCT_EXTENT, no floor; optionally spheres among them."""
    rng = np.random.default_rng(seed)
    e = OCT_EXTENT - size
    c = rng.uniform(-e, e, size=(n, 1, 3)) + OCT_CENTRE
    tris = (c + rng.uniform(-size, size, size=(n, 3, 3))).astype(F).reshape(n, 9)
    rgb = rng.uniform(0.2, 1.0, size=(n, 3)).astype(F)
    if not n_spheres:
        return tris, rgb, {}
    r = rng.uniform(0.8, 2.4, size=(n_spheres, 1))
    sc = rng.uniform(-(OCT_EXTENT - 2.4), OCT_EXTENT - 2.4, size=(n_spheres, 3)) + OCT_CENTRE
    kinds = np.zeros(n + n_spheres, np.uint8)
    kinds[rng.choice(n + n_spheres, n_spheres, replace=False)] = 1
    return tris, rgb, dict(spheres=np.concatenate([sc, r], axis=1).astype(F),
                           sphere_rgb=rng.uniform(0.2, 1.0, size=(n_spheres, 3)).astype(F), kinds=kinds)


def prim_box(tris, extra):
    """The box of every primitive of a scene, spheres with their radius (f64; the float32 inputs are exact in it)."""
    v = tris.reshape(-1, 3).astype(np.float64)
    lo, hi = v.min(axis=0), v.max(axis=0)
    if extra:
        s = extra["spheres"].astype(np.float64)
        lo, hi = np.minimum(lo, (s[:, :3] - s[:, 3:]).min(axis=0)), np.maximum(hi, (s[:, :3] + s[:, 3:]).max(axis=0))
    return lo, hi


def light_in_octant(k):
    """A small light triangle whose every surface-to-light direction lies in octant k: its centre OCT_LIGHT_OFFSET
    beyond the soup's centre on each axis, on the side octant_signs(k) names."""
    centre = OCT_CENTRE + octant_signs(k) * OCT_LIGHT_OFFSET
    return (centre + np.array([[-2.0, 0.5, -1.5], [2.0, -0.5, -1.0], [0.0, 1.0, 2.0]])).astype(F).reshape(9)


def eye_in_octant(k):
    """Camera keywords for primary rays whose directions all lie in octant k: the eye on the soup's diagonal, on the
    side the directions come FROM, looking at the centre."""
    eye = OCT_CENTRE - octant_signs(k) * OCT_EYE_OFFSET
    return dict(eye=tuple(float(x) for x in eye), look_at=tuple(float(x) for x in OCT_CENTRE), up=(0.0, 1.0, 0.0),
                distance=OCT_DISTANCE)


# (eye octant, light octant, spheres): every octant twice as the eye's and twice as the light's; half carry spheres
OCTANT_CASES = [(k, k ^ 7, bool(k & 1)) for k in range(8)] + [(k, k ^ 6, not (k & 1)) for k in range(8)]


def octant_scene(eye_oct, light_oct, with_spheres):
    """-> (name, W, H, tris, rgb, extra, keywords) for rtx.Scene / orc.Scene."""
    tris, rgb, extra = octant_soup(100 + 8 * eye_oct + light_oct, n_spheres=100 if with_spheres else 0)
    kw = dict(eye_in_octant(eye_oct), light_tri=light_in_octant(light_oct), nb_light_sample=OCT_LIGHT_SAMPLES)
    name = "eye octant %d, light octant %d%s" % (eye_oct, light_oct, ", spheres" if with_spheres else "")
    return (name,) + OCT_FRAME + (tris, rgb, extra, kw)


GENERAL_CASES = ["light inside", "eye and light inside"]


def general_loop_scene(which):
    """The two scenes whose walks have no common octant.  'light inside': the eye outside on a diagonal, the light
    triangle at the soup's centre, so shadow rays leave the surfaces in every direction.  'eye and light inside':
    the eye inside the soup's box as well, looking along -z, in a frame whose centre (where the primary directions
    change sign on x and on y) lies inside an 8 x 8 tile, not between two."""
    light = (OCT_CENTRE + np.array([[-1.5, 0.4, -1.0], [1.5, -0.4, -1.2], [0.0, 0.8, 1.6]])).astype(F).reshape(9)
    W, H = OCT_FRAME
    if which == "light inside":
        tris, rgb, extra = octant_soup(301, n=1800, n_spheres=0)
        kw = dict(eye_in_octant(5), light_tri=light, nb_light_sample=OCT_LIGHT_SAMPLES)
    else:
        tris, rgb, extra = octant_soup(302, n=1800, n_spheres=100)
        W, H = W - 4, H - 4
        eye = OCT_CENTRE + np.array([0.0, 0.0, 12.0])
        kw = dict(eye=tuple(float(x) for x in eye), look_at=(float(eye[0]), float(eye[1]), float(eye[2]) - 1.0),
                  up=(0.0, 1.0, 0.0), distance=40.0, light_tri=light, nb_light_sample=OCT_LIGHT_SAMPLES)
    return which, W, H, tris, rgb, extra, kw


def primary_directions(rtx, W, H, samples, kw):
    """Every primary direction of a W x H frame, [H, W, 3], by tests/np_ref.py (create_rays, src/main.rs:151-178) with
    the camera basis of rtx.camera_new."""
    import np_ref
    cam = rtx.camera_new(kw["eye"], kw["look_at"], kw["up"])
    py, px = np.meshgrid(np.arange(H, dtype=np.uint32), np.arange(W, dtype=np.uint32), indexing="ij")
    _, d = np_ref.primary_rays(px.reshape(-1), py.reshape(-1), W, H, kw["eye"], cam, kw["distance"],
                               np.asarray(samples, F))
    return d.reshape(H, W, 3)


def hit_prim_boxes(tris, extra, otri):
    """Per pixel the box of the primitive the oracle's want_tri names (lo, hi: [H, W, 3], NaN where nothing is hit).
    The hit point lies in that box up to rounding, so a light beyond / short of it fixes the shadow rays' signs."""
    kinds = extra["kinds"] if extra else np.zeros(len(tris), np.uint8)
    v = tris.reshape(-1, 3, 3).astype(np.float64)
    lo, hi = np.zeros((len(kinds), 3)), np.zeros((len(kinds), 3))
    lo[kinds == 0], hi[kinds == 0] = v.min(axis=1), v.max(axis=1)
    if extra:
        s = extra["spheres"].astype(np.float64)
        lo[kinds == 1], hi[kinds == 1] = s[:, :3] - s[:, 3:], s[:, :3] + s[:, 3:]
    hit = otri != NO_HIT
    idx = np.where(hit, otri, 0).astype(np.int64)
    plo, phi = lo[idx], hi[idx]
    plo[~hit], phi[~hit] = np.nan, np.nan
    return plo, phi


def oracle_counts(ref, otri):
    """(primary hits, lit pixels, hit pixels that are black) of an oracle image and its want_tri plane."""
    hit = otri != NO_HIT
    lit = ref.max(axis=2) > 0
    return int(hit.sum()), int((hit & lit).sum()), int((hit & ~lit).sum())


# ---------------------------------------------------------------------------------------------- cut-vs-whole scenes
CUT_FRAME = (160, 120)


def _cut_soup(seed, n, centre, extent, size):
    g = np.random.default_rng(seed)
    c = g.uniform(-extent, extent, (n, 1, 3)) + np.asarray(centre, F)
    t = (c + g.uniform(-size, size, (n, 3, 3))).astype(F).reshape(n, 9)
    return t, g.uniform(0.2, 1.0, (n, 3)).astype(F)


def cut_scenes():
    """The three scenes of test_cut_and_whole_stream_walks_give_the_same_bytes: name -> Scene keywords, with 'tris' and
    'rgb' among them.  Built here so that the child processes and the parent render the same arrays."""
    out = {}
    # 1. the light INSIDE the mesh: the light's box overlaps every tile's hit box, shafts run in every direction
    t, c = _cut_soup(1, 3000, (0, 0, 0), 40, 2.5)
    out['light inside'] = dict(tris=t, rgb=c, eye=(0, 10, 150), look_at=(0, 0, 0), distance=90.0,
                               light_tri=np.array([-3, 1, -3, 3, 1, -3, 0, -2, 3], F), nb_light_sample=24)
    # 2. coordinates around one million: the margins of the shaft test are relative to the scene's magnitude
    t, c = _cut_soup(2, 2500, (1.0e6, 2.0e6, -1.5e6), 60, 4.0)
    floor = np.array([[1.0e6 - 500, 2.0e6 - 70, -1.5e6 + 500, 1.0e6 + 500, 2.0e6 - 70, -1.5e6 + 500, 1.0e6, 2.0e6 - 70, -1.5e6 - 800]], F)
    out['coordinates of a million'] = dict(tris=np.concatenate([t, floor]), rgb=np.concatenate([c, np.array([[0.5, 0.5, 0.5]], F)]),
                                            eye=(1.0e6, 2.0e6 + 30, -1.5e6 + 260), look_at=(1.0e6, 2.0e6 - 20, -1.5e6), distance=100.0,
                                            light_tri=np.array([1.0e6 - 15, 2.0e6 + 200, -1.5e6 - 10, 1.0e6 + 15, 2.0e6 + 200, -1.5e6 - 10, 1.0e6, 2.0e6 + 200, -1.5e6 + 12], F),
                                            nb_light_sample=20)
    # 3. spheres among the triangles, and two primary rays per pixel
    t, c = _cut_soup(3, 1500, (0, 30, 0), 50, 3.0)
    g = np.random.default_rng(33)
    sph = np.concatenate([g.uniform(-50, 50, (200, 3)) + np.array([0, 30, 0]), g.uniform(0.5, 4.0, (200, 1))], axis=1).astype(F)
    floor = np.array([[-400, -25, 300, 400, -25, 300, 0, -25, -600]], F)
    out['spheres, two primary rays'] = dict(tris=np.concatenate([t, floor]), rgb=np.concatenate([c, np.array([[0.5, 0.5, 0.5]], F)]),
                                             spheres=sph, sphere_rgb=g.uniform(0.2, 1.0, (200, 3)).astype(F),
                                             eye=(0, 60, 220), look_at=(0, 20, 0), distance=110.0, nb_ray=2, nb_light_sample=16)
    return out
