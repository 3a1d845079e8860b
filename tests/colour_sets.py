"""Fixtures for the colour tests — pixels whose linear value lies AT a gamma step, and primitive colours outside [0, 1]
(zeros of both signs, negatives, huge and tiny values, infinities, NaN) — with the CPU oracle's answers: numpy, the oracle
binding and the library's host side only, no GPU.

1. The gamma ladder.  The reference's ground triangle alone under main()'s camera and light, an 8 x 8 frame, one ray per
   pixel, 1 and 100 light samples.  11 of the 64 pixels see the ground (LADDER_PIXELS).  For every step b = 1..255 and both
   counts an entry holds two ADJACENT floats c_lo < c_hi and a pixel p: with the ground grey (c_hi, c_hi, c_hi) the oracle's
   linear value at p is exactly thr[b] (byte b), with c_lo it is the float just below thr[b] (byte b - 1).  The ordered
   f32 sum of a pixel is monotone in the colour, so the pair is found by bisection on the colour's bits; whether the two
   values are exactly those is chance per pixel, and the pixels are tried in turn until one lands.  The coloured ladder
   takes the grey one's colours three at a time: channels (r, g, b) carry the c_hi (then the c_lo) of steps b, b + 85,
   b + 170, each channel exact at its own step's pixel — the three searches of a pixel differ and no tile is grey.
   Both are stored in tests/golden/colour_ladder.json (bit patterns); write_ladder() recomputes the file.
   horizon(): the ground under a camera that grazes it, two rays per pixel, where a tile has hits on ray 0 and none on
   ray 1 — the pixels the scheduling pass stores from the running sums.

2. Colour classes (CLASSES).  A 24 x 16 frame of the size of prims_sets' yard — the ground, 39 more triangles, 18 spheres —
   laid out in the frame's six 8 x 8 tiles (LAYOUT) so that each tile is of a stated kind: every class sits on a quad and
   on a sphere.  Variants: the ground ordinary, grey 2^61, +inf (GROUND_VARIANTS); class_ladder(): 16 gamma steps at a
   pixel of an ordinary grey quad in the tile that holds the 2^61 grey; whole_stream(): the classes spread over
   gpu_forms.whole_stream_scene's soup.

tests/test_colour_sets.py states, without a GPU, the conditions these fixtures must meet; tests/test_gpu_colours.py uses
them.  Everything is built once per process (query_sets._once)."""
import json
import os

import numpy as np

import query_sets as qs
import view_sets as vs
from query_sets import F

HERE = os.path.dirname(os.path.abspath(__file__))
LADDER_PATH = os.path.join(HERE, "golden", "colour_ladder.json")
LADDER_COUNTS = (1, 100)
LADDER_W = LADDER_H = 8
# (x, y) of the ground pixels of the 8 x 8 frame, in the order the search tries them
LADDER_PIXELS = tuple((x, 7) for x in range(8)) + ((2, 6), (4, 6), (7, 6))
# Camera distances: main()'s, at which 253 of the 255 steps land exactly at one of the 11 pixels for both counts; steps 65
# and 214 with 100 samples land at none of them (the nearest values lie 1 ulp off on one side) and take a pixel of the same
# frame at half the distance, whose three lower rows see the ground: another pixel, not a looser condition
LADDER_DISTANCES = (288.0, 144.0)
NO_HIT = 0xFFFFFFFF


def f32(bits):
    return np.array([bits], np.uint32).view(F)[0]


def bits_of(x):
    return int(np.array([x], F).view(np.uint32)[0])


def below(x):
    """the float just below a positive float"""
    return f32(bits_of(x) - 1)


# ------------------------------------------------------------------------------------------------------ thresholds
def oracle_byte(orc, x):
    import ctypes as C
    c = np.full(3, x, F)
    out = (C.c_uint8 * 3)()
    orc.lib().orc_color_to_rgb8(orc._fp(c), out)
    return int(out[0])


def thresholds(orc):
    """thr[b], b = 1..255: the smallest float whose oracle byte is >= b, by bisection over the bits of [+0.0, 2.0];
    thr[0] = -inf as the library has it -> float32 [256]"""
    def make():
        thr = np.zeros(256, F)
        thr[0] = -np.inf
        assert oracle_byte(orc, F(2.0)) == 255 and oracle_byte(orc, F(0.0)) == 0
        for b in range(1, 256):
            lo, hi = 0, bits_of(2.0)                      # byte(lo) < b <= byte(hi)
            while hi - lo > 1:
                mid = (lo + hi) // 2
                if oracle_byte(orc, f32(mid)) >= b:
                    hi = mid
                else:
                    lo = mid
            thr[b] = f32(hi)
        thr.setflags(write=False)
        return thr
    return qs._once("colour_thr", make)


# ------------------------------------------------------------------------------------------------------ the ladder
def ground_scene(binding, samples, rgb, count, distance=LADDER_DISTANCES[0], **more):
    """either binding's Scene of the ground alone with the colour `rgb` (three floats), 8 x 8, one ray, `count` samples"""
    tris = np.asarray(binding.GROUND_TRI, F).reshape(1, 9)
    return binding.Scene(LADDER_W, LADDER_H, tris, np.asarray(rgb, F).reshape(1, 3), samples[:4096], nb_ray=1,
                         nb_light_sample=count, distance=distance, **more)


def ground_render(orc, samples, rgb, count, distance=LADDER_DISTANCES[0]):
    """-> (frame uint8 [8, 8, 3], lin float32 [8, 8, 3], tri uint32 [8, 8]) of the oracle"""
    osc = ground_scene(orc, samples, rgb, count, distance)
    frame, _, tri, lin = osc.render_rows(mode=orc.MODE_BVH, nthreads=1, want_tri=True, want_lin=True)
    osc.close()
    return frame, lin, tri


def ground_pixels(orc, samples, distance):
    """(x, y) of the frame's ground pixels at a camera distance, the lowest row first"""
    if distance == LADDER_DISTANCES[0]:
        return LADDER_PIXELS
    tri = ground_render(orc, samples, (0.5, 0.5, 0.5), 1, distance)[2]
    return tuple((int(x), int(y)) for y, x in np.argwhere(tri != NO_HIT)[::-1])


def ground_value(orc, samples, c, count, pixel, distance=LADDER_DISTANCES[0]):
    """the oracle's linear red at `pixel` = (x, y) with the ground grey c"""
    osc = ground_scene(orc, samples, (c, c, c), count, distance)
    v = osc.render_pixel(pixel[0], pixel[1])[0]
    osc.close()
    return F(v)


def bisect_onto(value_of, target, lo_bits=1, hi_bits=0x7F7FFFFF):
    """value_of: monotone (not strictly) from a positive float's bits to a float.  -> (bits of the smallest colour whose
    value is >= target) or None when even hi_bits stays below"""
    if not value_of(hi_bits) >= target:
        return None
    if value_of(lo_bits) >= target:
        return lo_bits
    lo, hi = lo_bits, hi_bits
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if value_of(mid) >= target:
            hi = mid
        else:
            lo = mid
    return hi


def ladder_entry(orc, samples, thr, step, count, distances=LADDER_DISTANCES):
    """the first pixel at which the bisected pair is exact on both sides -> dict(step, count, distance, pixel, c_lo, c_hi:
    bits) or None; and, for the report, how far (in ulps, c_lo's and c_hi's value) the pixels tried before it missed"""
    target = thr[step]
    want = (bits_of(target) - 1, bits_of(target))
    missed = []
    for distance in distances:
        for p in ground_pixels(orc, samples, distance):
            hi = bisect_onto(lambda b: ground_value(orc, samples, f32(b), count, p, distance), target)
            if hi is None:
                continue
            got = tuple(bits_of(ground_value(orc, samples, f32(c), count, p, distance)) for c in (hi - 1, hi))
            if got == want:
                return dict(step=step, count=count, distance=distance, pixel=list(p), c_lo=hi - 1, c_hi=hi), missed
            missed.append((distance, p, got[0] - want[0], got[1] - want[1]))
    return None, missed


def coloured_of(orc, samples, grey):
    """the coloured ladder of a grey one: per count and b = 1..85 the steps (b, b + 85, b + 170), their pixels, and the two
    colours (the three c_hi, the three c_lo).  The three pixels belong to one frame: where the grey entries' camera
    distances differ, the three steps are searched again at the farthest of them"""
    thr = thresholds(orc)
    out = []
    for count in LADDER_COUNTS:
        by_step = {e["step"]: e for e in grey if e["count"] == count}
        for b in range(1, 86):
            steps = [(b - 1 + k) % 255 + 1 for k in (0, 85, 170)]
            e = [by_step[s] for s in steps]
            distances = sorted(set(x["distance"] for x in e))
            if len(distances) != 1:
                e = [ladder_entry(orc, samples, thr, s, count, distances[:1])[0] for s in steps]
                if None in e:
                    raise RuntimeError("steps %s with %d samples do not all land at distance %g" % (steps, count, distances[0]))
            out.append(dict(steps=steps, count=count, distance=e[0]["distance"], pixels=[x["pixel"] for x in e],
                            rgb_lo=[x["c_lo"] for x in e], rgb_hi=[x["c_hi"] for x in e]))
    return out


def compute_ladder(orc, samples, steps=range(1, 256), counts=LADDER_COUNTS):
    thr = thresholds(orc)
    grey = []
    for count in counts:
        for step in steps:
            e, missed = ladder_entry(orc, samples, thr, step, count)
            if e is None:
                raise RuntimeError("step %d with %d samples lands exactly at none of the pixels: %s" % (step, count, missed))
            grey.append(e)
    return grey


def write_ladder(orc, samples, path=LADDER_PATH):
    """recomputes both ladders and writes tests/golden/colour_ladder.json"""
    grey = compute_ladder(orc, samples)
    doc = dict(about="tests/colour_sets.py: write_ladder().  Colours are float32 bit patterns; pixels are (x, y).",
               thresholds=[bits_of(t) for t in thresholds(orc)[1:]], grey=grey, coloured=coloured_of(orc, samples, grey))
    with open(path, "w") as f:
        f.write(json.dumps(doc, separators=(",", ":")).replace('},{', '},\n{') + "\n")
    return doc


def ladder():
    """the stored ladders: dict(thresholds = bits of thr[1..255], grey = [dict(step, count, distance, pixel, c_lo, c_hi)], coloured =
    [dict(steps, count, distance, pixels, rgb_lo, rgb_hi)])"""
    def make():
        with open(LADDER_PATH) as f:
            return json.load(f)
    return qs._once("colour_ladder", make)


def grey_colours(count, every=1):
    """[(what, rgb float32 [3], entry)] of the grey ladder for one count: every `every`-th step, c_hi then c_lo"""
    out = []
    for e in ladder()["grey"]:
        if e["count"] == count and (e["step"] - 1) % every == 0:
            for side in ("c_hi", "c_lo"):
                out.append(("grey step %d %s, %d samples" % (e["step"], side, count), np.full(3, f32(e[side]), F), e))
    return out


def coloured_colours(count):
    out = []
    for e in ladder()["coloured"]:
        if e["count"] == count:
            for side in ("rgb_hi", "rgb_lo"):
                out.append(("steps %s %s, %d samples" % (e["steps"], side, count), np.array(e[side], np.uint32).view(F), e))
    return out


def ladder_frames(orc, samples, count, kind, every=1):
    """the oracle's frames of one ladder for one count, each an oracle scene CREATED with the colour:
    [(what, rgb, frame, lin, entry)]"""
    def make():
        cols = grey_colours(count, every) if kind == "grey" else coloured_colours(count)
        out = []
        for what, rgb, e in cols:
            frame, lin, _ = ground_render(orc, samples, rgb, count, e["distance"])
            out.append((what, rgb, frame, lin, e))
        return out
    return qs._once("colour_ladder_frames_%d_%s_%d" % (count, kind, every), make)


# ------------------------------------------------------------------------------------------------------ the horizon
HORIZON_NB_RAY, HORIZON_COUNT = 2, 100
HORIZON_DISTANCES = tuple(420.0 + 0.5 * k for k in range(80))     # main()'s camera with a longer lens: the one with most such pixels
HORIZON_STEPS, HORIZON_STRIDE = 16, 15       # 16 steps: every 15th, or the next one after it that lands exactly


def ray_hits(orc, osc, width, height, camera, samples, nb_ray):
    """the hit primitive of every primary ray by orc_closest_hit on create_rays' rays -> uint32 [height, width, nb_ray]"""
    import shade_sets as ss
    o, d, _, _, _ = ss.camera_raw_rays(orc, width, height, camera["eye"], camera["look_at"], camera["up"], camera["distance"],
                                       samples[:4096], nb_ray)
    prim, _, _ = ss._closest(osc, o, ss.units_of(orc, d))
    return prim.reshape(height, width, nb_ray)


def horizon_camera(orc, distance):
    return dict(eye=orc.EYE, look_at=orc.LOOK_AT, up=orc.UP, distance=distance)


def horizon_scene(binding, samples, rgb, distance, **more):
    tris = np.asarray(binding.GROUND_TRI, F).reshape(1, 9)
    return binding.Scene(LADDER_W, LADDER_H, tris, np.asarray(rgb, F).reshape(1, 3), samples[:4096], nb_ray=HORIZON_NB_RAY,
                         nb_light_sample=HORIZON_COUNT, distance=distance, **more)


def horizon(orc, samples):
    """The ground alone through main()'s camera with a longer lens, so that the ground's far edge crosses the frame's last
    row: two rays per pixel, and in the frame's one tile some pixels' ray 0 meets the ground while NO ray 1 does.  The
    last ray's tile is then one without a hit, and the scheduling pass stores its pixels from the running sums.
    -> dict(distance, hits [8, 8, 2] primitive per ray, entries = HORIZON_STEPS ladder entries (ladder_entry's dict, the
    colour pair bisected at a pixel whose ray 0 hit), frames = [(what, rgb, frame, lin)] for c_hi and c_lo of each)"""
    def make():
        thr = thresholds(orc)
        best = None
        for d in HORIZON_DISTANCES:
            osc = horizon_scene(orc, samples, (0.5, 0.5, 0.5), d)
            h = ray_hits(orc, osc, LADDER_W, LADDER_H, horizon_camera(orc, d), samples, HORIZON_NB_RAY)
            osc.close()
            n = int((h[:, :, 0] != NO_HIT).sum())
            if (h[:, :, 1] == NO_HIT).all() and n > (best[0] if best else 0):
                best = (n, d, h)
        if best is None:
            raise RuntimeError("no distance gives a tile with hits on ray 0 alone")
        _, distance, hits = best
        pixels = [(int(x), int(y)) for y, x in np.argwhere(hits[:, :, 0] != NO_HIT)]

        def value(c, p):
            osc = horizon_scene(orc, samples, (c, c, c), distance)
            v = osc.render_pixel(p[0], p[1])[0]
            osc.close()
            return F(v)
        entries, step = [], 1
        while len(entries) < HORIZON_STEPS and step <= 255:
            target = thr[step]
            want = (bits_of(target) - 1, bits_of(target))
            for p in pixels:
                hi = bisect_onto(lambda b: value(f32(b), p), target)
                if hi is not None and tuple(bits_of(value(f32(c), p)) for c in (hi - 1, hi)) == want:
                    entries.append(dict(step=step, count=HORIZON_COUNT, distance=distance, pixel=list(p), c_lo=hi - 1, c_hi=hi))
                    step = HORIZON_STRIDE * ((step - 1) // HORIZON_STRIDE + 1) + 1
                    break
            else:
                step += 1
        frames = []
        for e in entries:
            for side in ("c_hi", "c_lo"):
                rgb = np.full(3, f32(e[side]), F)
                osc = horizon_scene(orc, samples, rgb, distance)
                frame, _, lin = osc.render_rows(mode=orc.MODE_BVH, nthreads=1, want_lin=True)
                osc.close()
                frames.append(("horizon step %d %s" % (e["step"], side), rgb, frame, lin))
        return dict(distance=distance, hits=hits, entries=entries, frames=frames)
    return qs._once("colour_horizon", make)


# ------------------------------------------------------------------------------------------------------ colour classes
FLT_MAX = np.finfo(F).max
SUBNORMAL = f32(0x00000123)
NAN = F(np.nan)
# name -> rgb.  "Grey and >= 0" is the kernels' grey-tile rule (-0.0 >= 0 holds; a NaN equals nothing)
CLASSES = {
    "+0": (0.0, 0.0, 0.0), "-0": (-0.0, -0.0, -0.0), "2^-61": (2.0 ** -61,) * 3, "subnormal": (SUBNORMAL,) * 3,
    "3": (3.0,) * 3, "40": (40.0,) * 3, "2^61": (2.0 ** 61,) * 3, "FLT_MAX": (FLT_MAX,) * 3, "+inf": (np.inf,) * 3,
    "grey": (0.3, 0.3, 0.3),
    "negative grey": (-0.4, -0.4, -0.4), "negative channel": (0.7, -0.2, 0.4), "-inf": (-np.inf,) * 3, "NaN grey": (NAN,) * 3,
    "NaN channel": (0.6, NAN, 0.2), "colour": (0.9, 0.4, 0.15),
}
GREY_CLASSES = ("+0", "-0", "2^-61", "subnormal", "3", "40", "2^61", "FLT_MAX", "+inf", "grey")
CLASS_FRAME = (24, 16)
CLASS_VIEW = (CLASS_FRAME, (0.0, 320.0, 240.0), (0.0, 0.0, 0.0), 40.0)
CLASS_CONFIGS = ((1, 4), (2, 4), (1, 100), (2, 100))         # (nb_ray, nb_light_sample)
QUAD_HEIGHT, SPHERE_HEIGHT, SPHERE_PIXELS = 8.0, 14.0, 0.95
GROUND_VARIANTS = {"ordinary": (0.5, 0.5, 0.5), "2^61": (2.0 ** 61,) * 3, "+inf": (np.inf,) * 3}
# The frame's six 8 x 8 tiles, each of 16 cells of 2 x 2 pixels; a cell holds a quad (two triangles in the plane
# y = QUAD_HEIGHT whose outline is the cell's) or a sphere (about SPHERE_PIXELS pixels in radius, at the cell's centre):
#   tile (0, 0)  grey and >= 0 throughout, with the 2^61 grey among ordinary greys, and the quad of the ladder beside it
#   tile (1, 0)  grey and >= 0 throughout: the other such classes
#   tile (2, 0)  the classes that are not: a mixed tile
#   tile (0, 1)  the ground, and one triangle a fifth of a pixel wide that ray 0 of ONE pixel meets and no other ray
#   tile (1, 1)  the ground with a negative grey and a -inf grey: grey throughout, but not >= 0
#   tile (2, 1)  open ground
# (kind, class, tile x, tile y, cell): kind "q" or "s"; cells are numbered row by row, 0..15
LAYOUT = tuple([("q", "2^61", 0, 0, 5), ("q", "grey", 0, 0, 6), ("q", "ladder", 0, 0, 9), ("s", "2^61", 0, 0, 10),
                ("s", "grey", 0, 0, 0), ("q", "40", 0, 0, 3), ("s", "40", 0, 0, 12), ("q", "3", 0, 0, 15), ("s", "3", 0, 0, 2)] +
               [(k, c, 1, 0, 2 * i + (k == "s")) for i, c in enumerate(("+0", "-0", "2^-61", "subnormal", "FLT_MAX", "+inf"))
                for k in ("q", "s")] +
               [(k, c, 2, 0, 2 * i + (k == "s")) for i, c in enumerate(("negative grey", "negative channel", "-inf", "NaN grey", "NaN channel", "colour"))
                for k in ("q", "s")] +
               [("q", "negative grey", 1, 1, 0), ("s", "negative grey", 1, 1, 1), ("q", "-inf", 1, 1, 4), ("s", "-inf", 1, 1, 5)])
SLIVER_PIXEL = (3, 11)                      # tile (0, 1): the pixel whose ray 0 meets the sliver
SLIVER_CLASS = "colour"
LADDER_CELL_RGB = (0.25, 0.25, 0.25)        # the ladder quad's colour where no ladder value is asked for
CLASS_LADDER_CONFIG = (1, 100)
CLASS_LADDER_STEPS, CLASS_LADDER_STRIDE = 16, 15


def _camera64(orc, view):
    u, v, w = (np.zeros(3, F) for _ in range(3))
    orc.lib().orc_camera_new(orc._fp(orc.f3(view[1])), orc._fp(orc.f3(view[2])), orc._fp(orc.f3(vs.UP)), orc._fp(u), orc._fp(v), orc._fp(w))
    return np.asarray(view[1], np.float64), u.astype(np.float64), v.astype(np.float64), w.astype(np.float64)


def _on_plane(cam, view, x, y, height):
    """the point of the plane y = height seen at frame position (x, y) (pixels, fractions allowed)"""
    eye, u, v, w = cam
    (fw, fh), _, _, distance = view
    d = (x - fw / 2.0) * u + (y - fh / 2.0) * v - distance * w
    return eye + d * ((height - eye[1]) / d[1])


def class_prims(orc, samples, ground="ordinary", ladder_rgb=LADDER_CELL_RGB):
    """the primitives of the class scene -> dict(tris, rgb, spheres, sphere_rgb, kinds, cls = class name per Vec position,
    ground = the ground's Vec position, ladder = the ladder quad's two Vec positions, sliver = the sliver's)"""
    import shade_sets as ss
    cam = _camera64(orc, CLASS_VIEW)
    tris, rgb, spheres, srgb, kinds, cls = [], [], [], [], [], []
    for kind, c, tx, ty, cell in LAYOUT:
        x0, y0 = 8 * tx + 2 * (cell % 4), 8 * ty + 2 * (cell // 4)
        colour = ladder_rgb if c == "ladder" else CLASSES[c]
        if kind == "q":
            p = [_on_plane(cam, CLASS_VIEW, x, y, QUAD_HEIGHT) for x, y in ((x0, y0), (x0 + 2, y0), (x0 + 2, y0 + 2), (x0, y0 + 2))]
            for a, b, d in ((0, 1, 2), (0, 2, 3)):
                tris.append(np.concatenate([p[a], p[b], p[d]]))
                rgb.append(colour)
                kinds.append(0)
                cls.append(c)
        else:
            centre = _on_plane(cam, CLASS_VIEW, x0 + 1.0, y0 + 1.0, SPHERE_HEIGHT)
            edge = _on_plane(cam, CLASS_VIEW, x0 + 1.0 + SPHERE_PIXELS, y0 + 1.0, SPHERE_HEIGHT)
            spheres.append(np.concatenate([centre, [np.linalg.norm(edge - centre)]]))
            srgb.append(colour)
            kinds.append(1)
            cls.append(c)
    # the sliver: around ray 0 of SLIVER_PIXEL, where it crosses the quads' plane
    o, d, _, px, py = ss.camera_raw_rays(orc, CLASS_FRAME[0], CLASS_FRAME[1], CLASS_VIEW[1], CLASS_VIEW[2], vs.UP, CLASS_VIEW[3],
                                         samples[:4096], 2)
    k = 2 * (SLIVER_PIXEL[1] * CLASS_FRAME[0] + SLIVER_PIXEL[0])
    d0 = d[k].astype(np.float64)
    at = cam[0] + d0 * ((QUAD_HEIGHT - cam[0][1]) / d0[1])
    tris.append(np.concatenate([at + (-1.0, 0.0, -0.6), at + (1.0, 0.0, -0.6), at + (0.0, 0.0, 1.2)]))
    rgb.append(CLASSES[SLIVER_CLASS])
    kinds.append(0)
    cls.append("sliver")
    tris.append(np.asarray(orc.GROUND_TRI, np.float64))
    rgb.append(GROUND_VARIANTS[ground])
    kinds.append(0)
    cls.append("ground")
    cls = np.array(cls)
    out = dict(tris=np.ascontiguousarray(np.array(tris, np.float64).astype(F)), rgb=np.ascontiguousarray(np.array(rgb, F)),
               spheres=np.ascontiguousarray(np.array(spheres, np.float64).astype(F)), sphere_rgb=np.ascontiguousarray(np.array(srgb, F)),
               kinds=np.array(kinds, np.uint8), cls=cls, ground=int(np.nonzero(cls == "ground")[0][0]),
               ladder=np.nonzero(cls == "ladder")[0], sliver=int(np.nonzero(cls == "sliver")[0][0]))
    return out


def ordinary_prims(prims):
    """the same primitives with ordinary colours in [0.2, 1): what a scene is uploaded with before a pose gives it the
    class colours"""
    rng = np.random.default_rng(5)
    return dict(prims, rgb=rng.uniform(0.2, 1.0, prims["rgb"].shape).astype(F), sphere_rgb=rng.uniform(0.2, 1.0, prims["sphere_rgb"].shape).astype(F))


def class_kw(prims, nb_ray, nb_light, **more):
    return dict(vs.camera(CLASS_VIEW), nb_ray=nb_ray, nb_light_sample=nb_light, spheres=prims["spheres"], sphere_rgb=prims["sphere_rgb"],
                kinds=prims["kinds"], **more)


def class_scene(binding, samples, prims, nb_ray, nb_light, frame=CLASS_FRAME, **more):
    return binding.Scene(frame[0], frame[1], prims["tris"], prims["rgb"], samples[:4096], **class_kw(prims, nb_ray, nb_light, **more))


def class_render(orc, samples, ground, nb_ray, nb_light, ladder_rgb=LADDER_CELL_RGB, light_tri=None):
    """an oracle scene CREATED with the class colours, rendered -> dict(prims, frame, lin, tri, stats, hits = the hit
    primitive per ray [16, 24, nb_ray])"""
    def make():
        prims = class_prims(orc, samples, ground, ladder_rgb)
        more = {} if light_tri is None else dict(light_tri=light_tri)
        osc = class_scene(orc, samples, prims, nb_ray, nb_light, **more)
        frame, st, tri, lin = osc.render_rows(mode=orc.MODE_BVH, want_tri=True, want_lin=True)
        hits = ray_hits(orc, osc, CLASS_FRAME[0], CLASS_FRAME[1], vs.camera(CLASS_VIEW), samples, nb_ray)
        osc.close()
        for a in (frame, lin, tri, hits):
            a.setflags(write=False)
        return dict(prims=prims, frame=frame, lin=lin, tri=tri, stats=st, hits=hits)
    key = "colour_class_%s_%d_%d_%s_%s" % (ground, nb_ray, nb_light, tuple(np.asarray(ladder_rgb, F).view(np.uint32)), light_tri)
    return qs._once(key, make)


def lit_table(orc, samples, ground, nb_ray, nb_light):
    """per primary ray with a hit, which of its light samples the oracle finds lit (main.rs:193-232 from oracle pieces)
    -> bool [16, 24, nb_ray, nb_light]"""
    import np_ref
    import shade_sets as ss

    def make():
        prims = class_prims(orc, samples, ground)
        osc = class_scene(orc, samples, prims, nb_ray, nb_light)
        w, h = CLASS_FRAME
        o, d, _, _, _ = ss.camera_raw_rays(orc, w, h, CLASS_VIEW[1], CLASS_VIEW[2], vs.UP, CLASS_VIEW[3], samples[:4096], nb_ray)
        prim, _, p_hit = ss._closest(osc, o, ss.units_of(orc, d))
        lp = ss.light_points(orc, orc.LIGHT_TRI, samples[:4096], nb_ray, nb_light)
        lit = np.zeros((len(o), nb_light), bool)
        for k in np.nonzero(prim != NO_HIT)[0]:
            r = k % nb_ray
            for i in range(nb_light):
                to_light = (lp[r, i] - p_hit[k]).astype(F)
                sd = qs.unit(orc, to_light)
                s = osc.closest_hit(p_hit[k], sd)
                far = np_ref._norm(np_ref._sub(np_ref._v(p_hit[k][None]), np_ref._v(np.array([list(s.p_hit)], F))))[0]
                lit[k, i] = (not s.hit) or far > np_ref._norm(np_ref._v(to_light[None]))[0]
        osc.close()
        return lit.reshape(h, w, nb_ray, nb_light)
    return qs._once("colour_lit_%s_%d_%d" % (ground, nb_ray, nb_light), make)


def tiles():
    """(tile x, tile y, row slice, column slice) of the frame's aligned 8 x 8 tiles"""
    return [(tx, ty, slice(8 * ty, 8 * ty + 8), slice(8 * tx, 8 * tx + 8)) for ty in range(CLASS_FRAME[1] // 8) for tx in range(CLASS_FRAME[0] // 8)]


def is_grey(rgb):
    """the kernels' rule for a hit pixel's colour: red == green == blue >= 0"""
    rgb = np.asarray(rgb, F)
    with np.errstate(invalid="ignore"):
        return (rgb[..., 0] == rgb[..., 1]) & (rgb[..., 1] == rgb[..., 2]) & (rgb[..., 0] >= 0)


def colour_at(prims):
    """rgb per Vec position"""
    out = np.zeros((len(prims["kinds"]), 3), F)
    out[prims["kinds"] == 0], out[prims["kinds"] == 1] = prims["rgb"], prims["sphere_rgb"]
    return out


def class_ladder(orc, samples):
    """CLASS_LADDER_STEPS entries of the grey ladder's kind at a pixel of the ladder quad — an ordinary grey in the tile
    that holds the 2^61 grey — under CLASS_LADDER_CONFIG: [(what, ladder_rgb float32 [3], entry)] for c_hi and c_lo"""
    def make():
        thr = thresholds(orc)
        nb_ray, nb_light = CLASS_LADDER_CONFIG
        base = class_render(orc, samples, "ordinary", nb_ray, nb_light)
        pixels = [(int(x), int(y)) for y, x in np.argwhere(np.isin(base["tri"], base["prims"]["ladder"]))]

        def value(c, p):
            osc = class_scene(orc, samples, class_prims(orc, samples, "ordinary", (c, c, c)), nb_ray, nb_light)
            v = osc.render_pixel(p[0], p[1])[0]
            osc.close()
            return F(v)
        out, step = [], 1
        while len(out) < 2 * CLASS_LADDER_STEPS and step <= 255:
            target = thr[step]
            want = (bits_of(target) - 1, bits_of(target))
            for p in pixels:
                hi = bisect_onto(lambda b: value(f32(b), p), target)
                if hi is not None and tuple(bits_of(value(f32(c), p)) for c in (hi - 1, hi)) == want:
                    e = dict(step=step, pixel=list(p), c_lo=hi - 1, c_hi=hi)
                    out += [("class ladder step %d %s" % (step, side), np.full(3, f32(e[side]), F), e) for side in ("c_hi", "c_lo")]
                    step = CLASS_LADDER_STRIDE * ((step - 1) // CLASS_LADDER_STRIDE + 1) + 1
                    break
            else:
                step += 1
        return out
    return qs._once("colour_class_ladder", make)


# ------------------------------------------------------------------------------------------------------ the whole stream
WHOLE_FRAME, WHOLE_LIGHT, WHOLE_SPHERES, WHOLE_NB_RAY = (40, 32), 8, 300, 2
WHOLE_GROUNDS = {"ordinary": (0.5, 0.5, 0.5), "2^61": (2.0 ** 61,) * 3, "NaN": (NAN,) * 3}


def whole_stream(orc, rtx, samples, ground):
    """gpu_forms.whole_stream_scene with the class colours spread over its soup and its spheres in turn, and the ground
    (the last triangle) one of WHOLE_GROUNDS; rendered by the oracle's leaf-gated brute force as test_gpu_kernel_forms
    renders that scene -> dict(tris, rgb, extra, frame, tri, stats)"""
    import gpu_forms as gf

    def make():
        tris, rgb, extra = gf.whole_stream_scene(rtx, n_spheres=WHOLE_SPHERES)
        table = np.array([CLASSES[c] for c in CLASSES], F)
        rgb = table[np.arange(len(rgb)) % len(table)].copy()
        rgb[-1] = WHOLE_GROUNDS[ground]
        extra = dict(extra, sphere_rgb=np.ascontiguousarray(table[(np.arange(WHOLE_SPHERES) + 5) % len(table)]))
        osc = orc.Scene(WHOLE_FRAME[0], WHOLE_FRAME[1], tris, rgb, samples, nb_ray=WHOLE_NB_RAY, nb_light_sample=WHOLE_LIGHT,
                        build_bvh=False, **extra)
        frame, st, tri = osc.render_rows(mode=orc.MODE_LEAFBOX, want_tri=True)
        osc.close()
        return dict(tris=tris, rgb=np.ascontiguousarray(rgb), extra=extra, frame=frame, tri=tri, stats=st, table=table)
    return qs._once("colour_whole_" + ground, make)
