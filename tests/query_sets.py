"""Ray sets for the ray-query tests, with the CPU oracle's answers: numpy and the oracle binding only, no GPU.

A set is (origins, second, expected RtxRayHit records, expected occlusion bytes or None): `second` holds directions for a
closest-hit call and targets for an occlusion call.  The expected records are orc_closest_hit(o, Ray::new(d)) per ray
(the normal is left zero: the GPU tests take it from the scene), the bytes main.rs:202,220-221 on those records.  Every
set is built once per process and shared by tests/test_query_sets.py (which states, without a GPU, the conditions a set
must meet to test what it is for) and tests/test_gpu_trace_rays_edges.py (which traces it)."""
import numpy as np

import np_ref
from test_host_spheres import mixed_scene

F = np.float32
NO_HIT = 0xFFFFFFFF
HIT_DTYPE = np.dtype([("prim", np.uint32), ("t", np.float32), ("p_hit", np.float32, 3), ("normal", np.float32, 3)])
LIGHT_POINT = (0.0, 300.0, -3.3)
BOX_LO, BOX_HI = (-150.0, 5.0, -120.0), (120.0, 250.0, 120.0)
W = H = 32
# camera and light of tests/test_gpu_spheres.py::test_mixed_soups
SOUP_VIEW = dict(eye=(0.0, 0.0, 0.0), look_at=(0.0, 0.0, -1.0), up=(0.0, 1.0, 0.0), distance=24.0,
                 light_tri=(-2.0, 9.0, -3.0, 2.0, 9.0, -3.0, 0.0, 9.0, 1.0), nb_light_sample=24)
# length_and_direction's gates (rtx_traverse.hpp): a wavefront takes the short sequences only while every lane has
# |component| >= 2^-45 and a squared length <= 2^100
COMPONENT_GATE, LENGTH2_GATE = F(2.0 ** -45), F(2.0 ** 100)
# One -0.0 direction component each, on the bunny: the reference's own tree rejects each at an ancestor box (a miss),
# while the +0.0 twin hits the primitive named here (tests/test_query_sets.py asserts both)
HARD_RAYS = {
    "x": ((-20.0, 200.0, 0.0), (-0.0, -1.0, 0.0)),
    "y": ((43.0, 75.0, -48.0), (0.0, -0.0, 1.0)),
    "z": ((-19.0, 115.0, -19.0), (0.0, -1.0, -0.0)),
}
HARD_TWIN_HITS = {"x": 3591, "y": 218, "z": 3601}
HARD_SLOTS = {"x": 0, "y": 127, "z": 149}      # lane 0 of group 0, lane 63 of group 1, the last lane of the partial group 2


def unit(orc, d):
    """Ray::new (ray.rs:12-17) by the oracle"""
    out = np.zeros(3, F)
    orc.lib().orc_ray_new(orc._fp(orc.f3(d)), orc._fp(out))
    return out


def oracle_hits(orc, osc, origins, directions, dtype):
    """orc_closest_hit(o, Ray::new(d)) per ray as RtxRayHit records (the normal is left zero), and the unit directions"""
    exp = np.zeros(len(origins), dtype)
    units = np.zeros((len(origins), 3), F)
    exp["prim"] = NO_HIT
    for i, (o, d) in enumerate(zip(origins, directions)):
        units[i] = unit(orc, d)
        h = osc.closest_hit(o, units[i])
        if h.hit:
            exp["prim"][i], exp["t"][i], exp["p_hit"][i] = h.tri, h.t, list(h.p_hit)
    return exp, units


def bits(a):
    return np.ascontiguousarray(a, dtype=F).view(np.uint32)


def check_hits(got, exp, normals, what):
    assert np.array_equal(got["prim"], exp["prim"]), "%s: primitives differ at %s" % (what, np.nonzero(got["prim"] != exp["prim"])[0][:8])
    assert np.array_equal(bits(got["t"]), bits(exp["t"])), what + ": t differs"
    assert np.array_equal(bits(got["p_hit"]), bits(exp["p_hit"])), what + ": p_hit differs"
    hit = exp["prim"] != NO_HIT
    if normals is not None:
        assert np.array_equal(bits(got["normal"][hit]), bits(normals[exp["prim"][hit]])), what + ": a triangle's normal differs"
    assert not got["t"][~hit].any() and not got["p_hit"][~hit].any() and not got["normal"][~hit].any(), what + ": a miss is not zeros"


def expected_occlusion(exp, origins, targets):
    """main.rs:202,220-221 on the oracle's closest hit, float32"""
    o, t = np_ref._v(origins), np_ref._v(targets)
    dist_light = np_ref._norm(np_ref._sub(t, o))
    dist_hit = np_ref._norm(np_ref._sub(o, np_ref._v(exp["p_hit"])))
    return ((exp["prim"] != NO_HIT) & ~(dist_hit > dist_light)).astype(np.uint8)


def check_normals(got, exp, stored, kinds, what):
    """a triangle's normal is the scene's stored one, a sphere's normalize(p_hit - origin) (sphere.rs:93-95; the stored
    row of a sphere is its origin), float32"""
    hit = exp["prim"] != NO_HIT
    sphere = np.zeros(len(exp), bool)
    sphere[hit] = kinds[exp["prim"][hit]] == 1
    tri = hit & ~sphere
    assert np.array_equal(bits(got["normal"][tri]), bits(stored[exp["prim"][tri]])), what + ": a triangle's normal differs"
    p = got["p_hit"][sphere]
    want = np.stack(np_ref._normalize(np_ref._sub(np_ref._v(p), np_ref._v(stored[exp["prim"][sphere]]))), axis=-1)
    assert np.array_equal(bits(got["normal"][sphere]), bits(want)), what + ": a sphere's normal differs"


def pair_sets(orc, osc, origins, targets):
    """point pairs as a closest-hit set along fl(target - origin) and as an occlusion set"""
    o, t = np.ascontiguousarray(origins, F), np.ascontiguousarray(targets, F)
    v = (t - o).astype(F)
    exp, _ = oracle_hits(orc, osc, o, v, HIT_DTYPE)
    return dict(trace=(o, v, exp, None), occlusion=(o, t, exp, expected_occlusion(exp, o, t)))


_built = {}


def _once(name, make):
    if name not in _built:
        _built[name] = make()
    return _built[name]


def bunny_random_sets(orc, osc, dtype=HIT_DTYPE):
    """1,500 random rays in a box around the bunny and 1,500 point pairs from the same origins (seed 7)"""
    def make():
        rng = np.random.default_rng(7)
        ro = rng.uniform(BOX_LO, BOX_HI, size=(1500, 3)).astype(F)
        rd = rng.normal(size=(1500, 3)).astype(F)
        sets = {"random": (ro, rd) + oracle_hits(orc, osc, ro, rd, dtype)}
        targets = rng.uniform(BOX_LO, BOX_HI, size=(1500, 3)).astype(F)
        rt = (targets - ro).astype(F)
        sets["random_targets"] = (ro, targets) + oracle_hits(orc, osc, ro, rt, dtype)
        return sets
    return _once("bunny_random", make)


def bunny(orc, samples):
    """big_bunny + ground as the oracle holds it, and the random sets"""
    def make():
        osc = orc.default_scene(["big_bunny.obj"], W, H, samples)
        return dict(osc=osc, sets=bunny_random_sets(orc, osc), ground=osc.n_tris - 1)
    return _once("bunny", make)


def scene_a(orc, samples):
    """220 triangles and 60 spheres interleaved in one Vec<Primitive> (tests/test_gpu_spheres.py::test_mixed_soups, seed 21)"""
    def make():
        tris, rgb, spheres, srgb, kinds = mixed_scene(np.random.default_rng(21), 220, 60)
        kw = dict(spheres=spheres, sphere_rgb=srgb, kinds=kinds, **SOUP_VIEW)
        osc = orc.Scene(W, H, tris, rgb, samples, **kw)
        r = spheres[:, 3:4]
        lo = np.minimum(tris.reshape(-1, 3).min(axis=0), (spheres[:, :3] - r).min(axis=0)).astype(F)
        hi = np.maximum(tris.reshape(-1, 3).max(axis=0), (spheres[:, :3] + r).max(axis=0)).astype(F)
        return dict(osc=osc, args=(W, H, tris, rgb, samples), kw=kw, kinds=kinds, spheres=spheres, lo=lo, hi=hi,
                    bound=float(max(np.abs(lo).max(), np.abs(hi).max())))
    return _once("scene_a", make)


def is_sphere(a, exp):
    out = np.zeros(len(exp), bool)
    hit = exp["prim"] != NO_HIT
    out[hit] = a["kinds"][exp["prim"][hit]] == 1
    return out


def inside_a_sphere(a, points):
    d = np.asarray(points, np.float64)[:, None, :] - a["spheres"][None, :, :3].astype(np.float64)
    return ((d * d).sum(axis=2) < a["spheres"][None, :, 3].astype(np.float64) ** 2).any(axis=1)


def set_a(orc, samples):
    """A: 1,000 point pairs drawn uniformly in the box of all primitives of scene A"""
    def make():
        a = scene_a(orc, samples)
        rng = np.random.default_rng(5)
        o = rng.uniform(a["lo"], a["hi"], size=(1000, 3)).astype(F)
        t = rng.uniform(a["lo"], a["hi"], size=(1000, 3)).astype(F)
        return pair_sets(orc, a["osc"], o, t)
    return _once("set_a", make)


def interleave(x, y):
    out = np.empty((2 * len(x),) + x.shape[1:], x.dtype)
    out[0::2], out[1::2] = x, y
    return out


def set_b(orc, samples):
    """B: 200 origins at 100 times scene A's largest coordinate magnitude, aimed at points in the inner half of its box;
    alone, and interleaved one for one with the first 200 pairs of set A"""
    def make():
        a = scene_a(orc, samples)
        rng = np.random.default_rng(12)
        u = rng.normal(size=(200, 3))
        u /= np.linalg.norm(u, axis=1)[:, None]
        o = (u * 100.0 * a["bound"]).astype(F)
        mid, quarter = 0.5 * (a["lo"] + a["hi"]), 0.25 * (a["hi"] - a["lo"])
        t = rng.uniform(mid - quarter, mid + quarter, size=(200, 3)).astype(F)
        far = pair_sets(orc, a["osc"], o, t)
        near = set_a(orc, samples)
        mixed = {}
        for k in ("trace", "occlusion"):
            f, n = far[k], near[k]
            mixed[k] = (interleave(f[0], n[0][:200]), interleave(f[1], n[1][:200]), interleave(f[2], n[2][:200]),
                        None if f[3] is None else interleave(f[3], n[3][:200]))
        return dict(far=far, mixed=mixed)
    return _once("set_b", make)


def positive_twin(d):
    """the same direction with +0.0 for every -0.0"""
    d = np.array(d, F)
    d[(d == 0) & np.signbit(d)] = 0.0
    return d


def hard_occlusion_pair(origin, direction, reach=F(50.0)):
    """target - origin keeps a -0.0 only as (-0.0) - (+0.0): the origin moves to +0.0 on the axis of the -0.0 component
    and the target has -0.0 there"""
    o, d = np.array(origin, F), np.array(direction, F)
    axis = (d == 0) & np.signbit(d)
    o[axis] = 0.0
    t = (o + d * reach).astype(F)
    t[axis] = -0.0
    return o, t


def far_origin_ray():
    """ray 0 of test_origins_far_outside_the_scene[100]"""
    rng = np.random.default_rng(11 + 100)
    u = rng.normal(size=(200, 3))
    u /= np.linalg.norm(u, axis=1)[:, None]
    o = (u * 100 * 1e4).astype(F)
    target = rng.uniform((-90.0, 35.0, -60.0), (60.0, 180.0, 55.0), size=(200, 3)).astype(F)
    return o[0], target[0]


def set_c(orc, samples):
    """C: groups holding hard rays (a -0.0 direction component).
    bunny     150 random rays, three of them replaced by a hard ray each, -0.0 in x / y / z, at slots 0, 127 and 149
    scene_a   the first 63 rays of set A and one hard ray
    both      62 random rays on the bunny, a far origin in lane 17 and a hard ray in lane 40"""
    def make():
        b, a = bunny(orc, samples), scene_a(orc, samples)
        out = {}
        ro, rd, rexp, _ = b["sets"]["random"]
        _, rt, texp, _ = b["sets"]["random_targets"]
        want = expected_occlusion(texp, ro, rt)

        o, d, exp = ro[:150].copy(), rd[:150].copy(), rexp[:150].copy()
        oo, ot, oexp, owant = ro[:150].copy(), rt[:150].copy(), texp[:150].copy(), want[:150].copy()
        for axis, slot in HARD_SLOTS.items():
            o[slot], d[slot] = HARD_RAYS[axis]
            exp[slot] = oracle_hits(orc, b["osc"], o[slot:slot + 1], d[slot:slot + 1], HIT_DTYPE)[0][0]
            oo[slot], ot[slot] = hard_occlusion_pair(*HARD_RAYS[axis])
            pair = pair_sets(orc, b["osc"], oo[slot:slot + 1], ot[slot:slot + 1])["occlusion"]
            oexp[slot], owant[slot] = pair[2][0], pair[3][0]
        out["bunny"] = dict(trace=(o, d, exp, None), occlusion=(oo, ot, oexp, owant))

        so, sd, sexp, _ = set_a(orc, samples)["trace"]
        _, st, _, swant = set_a(orc, samples)["occlusion"]
        ho, hd = np.array([[0.5, -0.25, 0.0]], F), np.array([[0.0, -0.0, -1.0]], F)
        o, d = np.concatenate([so[:63], ho]), np.concatenate([sd[:63], hd])
        exp = np.concatenate([sexp[:63], oracle_hits(orc, a["osc"], ho, hd, HIT_DTYPE)[0]])
        po, pt = hard_occlusion_pair(ho[0], hd[0], reach=F(12.0))
        pair = pair_sets(orc, a["osc"], po[None], pt[None])["occlusion"]
        out["scene_a"] = dict(trace=(o, d, exp, None),
                              occlusion=(np.concatenate([so[:63], pair[0]]), np.concatenate([st[:63], pair[1]]),
                                         np.concatenate([sexp[:63], pair[2]]), np.concatenate([swant[:63], pair[3]])))

        fo, ft = far_origin_ray()
        o, d, exp = ro[:64].copy(), rd[:64].copy(), rexp[:64].copy()
        oo, ot, oexp, owant = ro[:64].copy(), rt[:64].copy(), texp[:64].copy(), want[:64].copy()
        far = pair_sets(orc, b["osc"], fo[None], ft[None])
        o[17], d[17], exp[17] = far["trace"][0][0], far["trace"][1][0], far["trace"][2][0]
        oo[17], ot[17], oexp[17], owant[17] = (far["occlusion"][k][0] for k in range(4))
        o[40], d[40], exp[40] = out["bunny"]["trace"][0][0], out["bunny"]["trace"][1][0], out["bunny"]["trace"][2][0]
        oo[40], ot[40], oexp[40], owant[40] = (out["bunny"]["occlusion"][k][0] for k in range(4))
        out["both"] = dict(trace=(o, d, exp, None), occlusion=(oo, ot, oexp, owant))
        return out
    return _once("set_c", make)


def edge_targets(orc, osc, origins, exp):
    """D: for the rays of a set that hit, three targets each: p_hit, p_hit one ulp toward the origin in every coordinate,
    p_hit one ulp away from it; expected bytes from the oracle's closest hit along fl(target - origin)"""
    hit = exp["prim"] != NO_HIT
    o, p = np.ascontiguousarray(origins[hit]), np.ascontiguousarray(exp["p_hit"][hit])
    beyond = (F(2.0) * p - o).astype(F)
    out = {}
    for name, t in (("at", p), ("toward", np.nextafter(p, o)), ("away", np.nextafter(p, beyond))):
        assert t.dtype == F
        out[name] = pair_sets(orc, osc, o, t)["occlusion"]
    return dict(targets=out, first_prim=exp["prim"][hit])


def set_d(orc, samples):
    def make():
        b, a = bunny(orc, samples), scene_a(orc, samples)
        ro, _, rexp, _ = b["sets"]["random"]
        so, _, sexp, _ = set_a(orc, samples)["trace"]
        return dict(bunny=edge_targets(orc, b["osc"], ro, rexp), scene_a=edge_targets(orc, a["osc"], so, sexp))
    return _once("set_d", make)


SCALES = {"2^-60": -60, "2^-36": -36, "2^49": 49, "2^52": 52}
ONE_LANE_SLOTS = (5, 64 + 63, 128, 192 + 31)       # one ray of each group of 64
THIN_SLOTS = tuple(range(2, 128, 8))


def set_e(orc, samples):
    """E: directions multiplied by a power of two: Ray::new gives the unscaled direction's unit vector (asserted by
    tests/test_query_sets.py), so the expected records are the unscaled rays'.
    trace       the first 256 random rays of the bunny at each of SCALES, and `one_lane`: the rays of ONE_LANE_SLOTS at
                2^-60, the other 252 unscaled.  A component of a normal draw is below 2^-9 — what 2^-36 scales below the
                component gate — once in 640 draws (7 rays of the random set's 1,500), so in the `2^-36` batch the
                directions of THIN_SLOTS, 16 slots of groups 0 and 1, are the first normal draws of seed 36 that have
                such a component (origins kept); groups 2 and 3 are the random set's
    occlusion   target = origin + scaled direction, where the sum keeps the pair's meaning: 2^49 and 2^52 (a target far
                beyond the scene: the origin is absorbed, fl(target - origin) is the scaled direction within rounding),
                and `one_lane`: the rays of ONE_LANE_SLOTS at 2^52, the others at 2^6.  (At 2^-36 and 2^-60 the sum is
                the origin itself: a zero-length direction, outside the contract.)"""
    def make():
        b = bunny(orc, samples)
        ro, rd, rexp, _ = b["sets"]["random"]
        trace, occlusion = {}, {}
        unscaled = {name: rd[:256] for name in list(SCALES) + ["one_lane"]}
        records = {name: rexp[:256] for name in unscaled}
        draws = np.random.default_rng(36).normal(size=(20000, 3)).astype(F)
        thin = draws[np.abs(draws).min(axis=1) < F(2.0 ** -9)][:len(THIN_SLOTS)]
        unscaled["2^-36"], records["2^-36"] = rd[:256].copy(), rexp[:256].copy()
        unscaled["2^-36"][list(THIN_SLOTS)] = thin
        records["2^-36"][list(THIN_SLOTS)] = oracle_hits(orc, b["osc"], ro[list(THIN_SLOTS)], thin, HIT_DTYPE)[0]
        for name, k in SCALES.items():
            trace[name] = (ro[:256], (unscaled[name] * F(2.0 ** k)).astype(F), records[name], None)
        factor = np.ones((256, 1), F)
        factor[list(ONE_LANE_SLOTS)] = F(2.0 ** -60)
        trace["one_lane"] = (ro[:256], (rd[:256] * factor).astype(F), rexp[:256], None)
        factor = np.full((256, 1), F(64.0), F)
        factor[list(ONE_LANE_SLOTS)] = F(2.0 ** 52)
        for name, f in (("2^49", F(2.0 ** 49)), ("2^52", F(2.0 ** 52)), ("one_lane", factor)):
            occlusion[name] = pair_sets(orc, b["osc"], ro[:256], (ro[:256] + (rd[:256] * f).astype(F)).astype(F))["occlusion"]
        return dict(trace=trace, occlusion=occlusion, unscaled=unscaled)
    return _once("set_e", make)


def length2(v):
    """the kernels' float32 squared length: (x*x + y*y) + z*z"""
    v = np.asarray(v, F)
    return (v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2]


def takes_the_long_way(v):
    """per ray: would this lane send its wavefront through sqrtf and the divisions"""
    return (np.abs(np.asarray(v, F)).min(axis=1) < COMPONENT_GATE) | ~(length2(v) <= LENGTH2_GATE)
