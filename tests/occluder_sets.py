"""Scenes for the shadow walk's distance test (csrc/rtx_traverse.hpp: candidate_occludes, candidate_occludes_voted), with
the CPU oracle's answers: numpy and the oracle binding only, no GPU.

The walk settles a candidate from its distance t alone where t and the light's distance do not nearly coincide, and
evaluates the reference's expression (main.rs:220-221) where they do.  Four fixtures, one wall seen by an axis camera and
a light off to its side:
  (a) `below`     a 24-triangle sheet four units in front of the wall, the light twenty and more away: every candidate is an
                  occluder, and certified one
  (b) `beyond`    one triangle BEHIND the light along every shadow ray: every candidate is certified not to occlude, and
                  every sample is lit
  (c) `coplanar`  a triangle in the plane of the light's own triangle and around it: every candidate arrives with t within
                  a few ulp of the light's distance
  (d) `tile`      one 8 x 8 frame with the sheet of (a) over part of it and the triangle of (c): the 64 rays of a light
                  point hold settled and unsettled candidates side by side
tests/test_occluder_sets.py states, from the oracle alone, the conditions each must meet; tests/test_gpu_occluder_distance.py
traces them.  float32 restatements of both sides of the distance test are here for the two of them and for
tests/test_occluder_certificate.py."""
import numpy as np

import np_ref
import query_sets as qs
import shade_sets as ss

F = np.float32
NO_HIT = qs.NO_HIT
CAMERA = dict(eye=(0.0, 0.0, 0.0), look_at=(0.0, 0.0, -1.0), up=(0.0, 1.0, 0.0))
WALL = (-60.0, -40.0, -20.0, 60.0, -40.0, -20.0, 0.0, 80.0, -20.0)
# Light::get_sample's weights (triangle.rs:113-127: 1 - sqrt(u), sqrt(u) (1 - sqrt(v)), v sqrt(u)) do not add up to one:
# a light point is a point of the light's triangle scaled towards the world's origin by up to a quarter.  So the light's
# triangle lies in a plane THROUGH the origin, x + 3z = 0, which then holds every light point, and COVER lies in that plane
# around all of them (x from 15 to 39).  The eye is in that plane too and sees COVER edge on: no primary ray hits it.
LIGHT = (30.0, -2.0, -10.0, 30.0, 2.0, -10.0, 27.0, 0.0, -9.0)
COVER = (39.0, -12.0, -13.0, 39.0, 12.0, -13.0, 15.0, 0.0, -5.0)
BEYOND = (45.0, -200.0, -200.0, 45.0, 200.0, -200.0, 45.0, 0.0, 300.0)
NB_LIGHT = 8
K_UP, K_DOWN = F(1.0) + F(2.0 ** -20), F(1.0) - F(2.0 ** -20)


# ------------------------------------------------------------------------------------- both sides of the distance test
def exact_occludes(o, d, t, limit):
    """candidate_occludes: !(distance(orig, orig + t * dir) > dist_light), bvh.rs:69 and main.rs:220-221, float32, one
    rounding per operation.  o, d: [n, 3]; t, limit: [n]"""
    o, d, t, limit = (np.asarray(x, F) for x in (o, d, t, limit))
    with np.errstate(all="ignore"):
        q = [o[:, c] - (o[:, c] + t * d[:, c]) for c in range(3)]
        return ~(np.sqrt(np_ref._dot(q, q)) > limit)


def fma32(a, b, c):
    """fl32(a * b + c): the product of two float32 is exact in float64; the sum's rounding to float64 before the one to
    float32 moves the result in about one case in 2^29, by one ulp, far inside the certificate's margins"""
    return (np.asarray(a, F).astype(np.float64) * np.asarray(b, F).astype(np.float64) + np.asarray(c, F).astype(np.float64)).astype(F)


def certificate(o, t, limit):
    """candidate_occludes_voted's two comparisons -> (yes, no): the candidate certainly occludes / certainly does not.
    Neither: undecided, the exact expression answers."""
    o, t, limit = np.asarray(o, F), np.asarray(t, F), np.asarray(limit, F)
    cs = F(2.0 ** -22) * ((np.abs(o[:, 0]) + np.abs(o[:, 1])) + np.abs(o[:, 2]))
    with np.errstate(all="ignore"):
        return fma32(t, K_UP, cs) <= limit, fma32(t, K_DOWN, -cs) > limit


# ------------------------------------------------------------------------------------------------------- the fixtures
def sheet(seed=5, nx=3, ny=4, x=(6.0, 14.0), y=(-12.0, 12.0), z=-16.0):
    """nx x ny quads, two triangles each, four units in front of the wall, where their shadow falls on the part of the wall
    the eye sees beside them; the corners' depth jittered by up to 0.25"""
    rng = np.random.default_rng(seed)
    gx, gy = np.linspace(x[0], x[1], nx + 1), np.linspace(y[0], y[1], ny + 1)
    gz = z + rng.uniform(-0.25, 0.25, size=(nx + 1, ny + 1))
    p = lambda i, j: (gx[i], gy[j], gz[i, j])
    tris = []
    for i in range(nx):
        for j in range(ny):
            tris.append(p(i, j) + p(i + 1, j) + p(i + 1, j + 1))
            tris.append(p(i, j) + p(i + 1, j + 1) + p(i, j + 1))
    return np.array(tris, F)


def fixture(name, nb_ray=1, sphere=False):
    """-> dict(W, H, tris, rgb, extra, kw): the arguments of rtx.Scene / orc.Scene.  sphere: one sphere behind the wall,
    which no ray meets — the kernels' sphere forms on the same pixels"""
    wall = np.array([WALL], F)
    parts = dict(below=[sheet(), wall], beyond=[np.array([BEYOND], F), wall], coplanar=[np.array([COVER], F), wall],
                 tile=[sheet(), np.array([COVER], F), wall])[name]
    tris = np.ascontiguousarray(np.concatenate(parts))
    rng = np.random.default_rng(11)
    rgb = rng.uniform(0.3, 1.0, size=(len(tris), 3)).astype(F)
    W = H = 8 if name == "tile" else 32
    kw = dict(CAMERA, distance=6.0 if name == "tile" else 24.0, light_tri=LIGHT, nb_ray=nb_ray, nb_light_sample=NB_LIGHT)
    extra = {}
    if sphere:
        extra = dict(spheres=np.array([[0.0, 0.0, -40.0, 3.0]], F), sphere_rgb=np.array([[0.9, 0.2, 0.2]], F))
    return dict(name=name, W=W, H=H, tris=tris, rgb=rgb, extra=extra, kw=kw)


FIXTURES = ("below", "beyond", "coplanar", "tile")
_built = {}


def shadow_rays(orc, samples, name):
    """The shadow rays of fixture `name`'s frame (one primary ray per pixel) with the oracle's answers, built once:
    origins / targets [n, 3] (a pixel's hit point, a light point; pixel-major), unit [n, 3] Ray::new(target - origin),
    limit [n] the light's distance, prim / t [n] the oracle's closest hit along the ray, occluded [n] main.rs:220 on
    it, image the oracle's frame"""
    if name in _built:
        return _built[name]
    f = fixture(name)
    osc = orc.Scene(f["W"], f["H"], f["tris"], f["rgb"], samples, **f["kw"])
    o, raw, _, _, _ = ss.camera_raw_rays(orc, f["W"], f["H"], CAMERA["eye"], CAMERA["look_at"], CAMERA["up"], f["kw"]["distance"], samples)
    prim, _, p_hit = ss._closest(osc, o, ss.units_of(orc, raw))
    lp = ss.light_points(orc, LIGHT, samples, 1, NB_LIGHT)[0]
    hit = np.nonzero(prim != NO_HIT)[0]
    origins = np.repeat(p_hit[hit], NB_LIGHT, axis=0)
    targets = np.tile(lp, (len(hit), 1))
    pair = qs.pair_sets(orc, osc, origins, targets)["occlusion"]
    to_light = (targets - origins).astype(F)
    image, _ = osc.render_rows(mode=orc.MODE_BVH)
    out = dict(fixture=f, origins=origins, targets=targets, unit=ss.units_of(orc, to_light), limit=np_ref._norm(np_ref._v(to_light)),
               prim=pair[2]["prim"], t=pair[2]["t"], occluded=pair[3], pixel=np.repeat(hit, NB_LIGHT), image=image,
               primary_prim=prim)
    osc.close()
    _built[name] = out
    return out


def candidates_on(tri9, origins, unit):
    """Triangle::intersect and the leaf rule for one triangle, float32 (np_ref) -> (candidate [n], t [n])"""
    tr = np_ref.Tris(np.asarray(tri9, F).reshape(1, 9))
    o = tuple(origins[:, k:k + 1] for k in range(3))
    d = tuple(unit[:, k:k + 1] for k in range(3))
    some, t = np_ref.mt_intersect(tr, o, d)
    with np.errstate(all="ignore"):
        ok = some & ~(t < F(1.0)) & np_ref.slab(tuple(x[None, :] for x in tr.bmin), tuple(x[None, :] for x in tr.bmax), o, d)
    return ok[:, 0], t[:, 0]
