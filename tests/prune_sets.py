"""Scenes and rays on which a closest-hit walk that prunes by distance is wrong (csrc/rtx_traverse.hpp: advance_to_leaf
had such a form, PRUNE, until these rays were traced), with the CPU oracle's answers: numpy, the
oracle binding and the library's host-side scene read-back only, no GPU.

The reference never prunes by distance: its answer is the minimum of the COMPUTED distances of every accepted candidate.
For a ray nearly parallel to a triangle, Moeller-Trumbore's determinant is mostly rounding noise, u, v and t all carry
the same wrong factor, and the candidate is accepted with a distance far from where the triangle lies — for instance
in front of a wall that the triangle is behind.  A walk that has met the wall and leaves out every box entered beyond
the wall's distance never tests that triangle.

    emulate()        one wavefront's closest-hit walk over a stream as Scene.nodes() / primary_nodes() return it, on the
                     CPU: pre-order with the skip links, the global leaf first (walk_stream).  Candidates are the
                     oracle's (orc_triangle_intersect / orc_sphere_intersect, t >= 1, orc_bbox_intersect on the
                     primitive's own box), ties go to the higher reference leaf rank.  A box is visited when some lane
                     passes it.  With prune=True a lane only passes a box it enters no farther than its closest hit so
                     far — the rule the kernel had, stated MORE LENIENTLY, so that whatever is pruned here that kernel
                     pruned: the entry in float64 into the box widened by 2 cull_delta (the kernel's planes are moved by
                     one cull_delta and its float32 distances err by less than another), against best * (1 + 2^-15)
                     (the kernel: 1 + 2^-16).
    exposed          a ray whose unpruned emulation is the oracle's closest hit and whose pruned emulation names
                     another primitive: the oracle's primitive lies in a leaf the pruned walk does not open.

Scenes: a wall of 32 triangles at z = -100, seen from the origin, and behind it ill-conditioned triangles (planes that
miss the origin by 1e-6 .. 1e-2), four well-conditioned ones and optionally a sphere; in front of it two ill-conditioned
triangles whose distance may come out BEHIND the wall.  Each scene is built as it is and mirrored in z (rays mirrored
too, the light kept): the light orders the children of the library's tree, so the two walk the stream in different
orders.  Everything is drawn from fixed seeds and built once per process (query_sets._once).

tests/test_prune_sets.py states, without a GPU, the conditions these fixtures must meet; tests/test_gpu_prune.py traces,
shades and renders them."""
import ctypes as C

import numpy as np

import np_ref
import query_sets as qs
import shade_sets as ss
from query_sets import F, NO_HIT

LEAF, INDEX = 0x80000000, 0x3FFFFFFF          # scene_prep.h: kLeafFlag, kLeafIndexMask
WALL_Z, WALL_HALF, WALL_CELLS = -100.0, 160.0, 4
# (seed, index of the draw) of the ill-conditioned triangles behind the wall: draws of ill_triangle() towards which a
# large share of the rays from the origin is exposed (found by a search with np_ref; stated by tests/test_prune_sets.py)
BEHIND = ((5, 3), (2, 5), (1, 1), (1, 7), (2, 3), (3, 1))
FRONT = ((5, 3), (7, 4))                     # draws at 0.38 of the size: between the origin and the wall, z = -38 .. -99
FRONT_SCALE = 0.38
N_DRAWS = 800                                # rays drawn towards the triangle the exposed batches are taken from
N_EXPOSED = 128
SPHERE_BEHIND = (25.0, -35.0, -230.0, 28.0)
LIGHT_TRI = (-10.0, 40.0, -420.0, 10.0, 40.0, -420.0, 0.0, 55.0, -400.0)     # behind everything: the as-built wall goes first
NB_LIGHT = 6
EYE = (0.0, 0.0, 0.0)
ORDERS = ("built", "mirrored")
FRAME_DISTANCE = 10.0


# ---------------------------------------------------------------------------------------------------------- geometry
def ill_triangle(rng, scale=1.0):
    """a triangle whose plane misses the origin by 1e-6 .. 1e-2: vertices 101 a, 160 b, 260 (a + b) / 2 + 30 (a - b), moved
    along the plane's normal; a, b = (U(-.2, .2), U(-.2, .2), -1)"""
    a = np.array([rng.uniform(-.2, .2), rng.uniform(-.2, .2), -1.0])
    b = np.array([rng.uniform(-.2, .2), rng.uniform(-.2, .2), -1.0])
    n = np.cross(a, b)
    off = n / np.linalg.norm(n) * 10.0 ** rng.uniform(-6.0, -2.0)
    v = np.stack([101.0 * a, 160.0 * b, 260.0 * (a + b) / 2.0 + 30.0 * (a - b)]) * scale + off
    return v.reshape(9).astype(F)


def drawn_triangle(seed, index, scale=1.0):
    rng = np.random.default_rng(seed)
    for _ in range(index):
        ill_triangle(rng)
    return ill_triangle(rng, scale)


def wall():
    xs = np.linspace(-WALL_HALF, WALL_HALF, WALL_CELLS + 1)
    out = []
    for i in range(WALL_CELLS):
        for j in range(WALL_CELLS):
            x0, x1, y0, y1 = xs[i], xs[i + 1], xs[j], xs[j + 1]
            out += [[x0, y0, WALL_Z, x1, y0, WALL_Z, x1, y1, WALL_Z], [x0, y0, WALL_Z, x1, y1, WALL_Z, x0, y1, WALL_Z]]
    return np.array(out, F)


def well_conditioned():
    """four triangles behind the wall that face the origin"""
    out = []
    for k, (cx, cy, z) in enumerate(((-40.0, 30.0, -140.0), (35.0, 25.0, -150.0), (-30.0, -40.0, -170.0), (45.0, -20.0, -190.0))):
        out.append([cx - 25.0, cy - 20.0, z, cx + 25.0, cy - 20.0, z - 3.0 - k, cx, cy + 25.0, z + 2.0])
    return np.array(out, F)


def primitives(with_sphere):
    """-> (tris, rgb, keywords with the sphere arm or empty, groups: name -> primitive indices)"""
    parts = [wall(), np.stack([drawn_triangle(*d) for d in BEHIND]), well_conditioned(),
             np.stack([drawn_triangle(*d, scale=FRONT_SCALE) for d in FRONT])]
    names = ("wall", "behind", "well", "front")
    groups, at = {}, 0
    for name, p in zip(names, parts):
        groups[name] = np.arange(at, at + len(p))
        at += len(p)
    tris = np.ascontiguousarray(np.concatenate(parts))
    rgb = np.random.default_rng(77).uniform(0.2, 1.0, size=(len(tris), 3)).astype(F)
    extra = {}
    if with_sphere:
        extra = dict(spheres=np.array([SPHERE_BEHIND], F), sphere_rgb=np.array([[0.9, 0.4, 0.3]], F))
        groups["sphere"] = np.array([at])
    return tris, rgb, extra, groups


def mirror(tris, extra):
    t = tris.copy()
    t[:, 2::3] = -t[:, 2::3]
    if extra:
        s = extra["spheres"].copy()
        s[:, 2] = -s[:, 2]
        extra = dict(extra, spheres=s)
    return t, extra


def mirrored_rays(v):
    v = np.array(v, F)
    v[..., 2] = -v[..., 2]
    return v


def points_on(tri9, rng, n):
    """n points of a triangle, uniformly (float64)"""
    uv = rng.uniform(size=(n, 2))
    su = np.sqrt(uv[:, 0:1])
    v = np.asarray(tri9, np.float64).reshape(3, 3)
    return (1.0 - su) * v[0] + su * (1.0 - uv[:, 1:2]) * v[1] + su * uv[:, 1:2] * v[2]


# ---------------------------------------------------------------------------------------------------------- scenes
class Built:
    """one scene in one order: the oracle's scene, the library's host-side preparation, the tables the emulation needs"""

    def __init__(self, rtx, orc, samples, tris, rgb, extra, groups, camera=None, frame=(8, 8)):
        kw = dict(eye=EYE, look_at=(0.0, 0.0, float(np.sign(tris[0, 2]))), up=(0.0, 1.0, 0.0), distance=FRAME_DISTANCE,
                  light_tri=LIGHT_TRI, nb_light_sample=NB_LIGHT, **extra)
        if camera:
            kw.update(camera)
        self.args, self.kw, self.groups = (frame[0], frame[1], tris, rgb, samples), kw, groups
        self.tris, self.rgb, self.extra = tris, rgb, extra
        self.osc = orc.Scene(*self.args, **kw)
        self.spheres = extra["spheres"] if extra else np.zeros((0, 4), F)
        self.n = len(tris) + len(self.spheres)
        self.kinds = np.concatenate([np.zeros(len(tris), np.uint8), np.ones(len(self.spheres), np.uint8)])
        with rtx.Scene(*self.args, **kw) as s:             # creation and read-back need no device
            self.info = s.info()
            self.nodes, self.order = s.nodes()
            self.primary, self.primary_own = s.primary_nodes()
        lo = np.concatenate([tris.reshape(-1, 3, 3).min(axis=1), self.spheres[:, :3] - self.spheres[:, 3:]])
        hi = np.concatenate([tris.reshape(-1, 3, 3).max(axis=1), self.spheres[:, :3] + self.spheres[:, 3:]])
        self.lo, self.hi = lo.astype(F), hi.astype(F)
        magnitude = max(float(np.abs(self.lo).max()), float(np.abs(self.hi).max()), float(np.abs(np.asarray(kw["eye"], F)).max()))
        self.cull_delta = magnitude * 2.0 ** -19                          # scene_prep.cpp: PreparedScene::cull_delta
        # Triangle::new's edges by the oracle; ranks of the reference's leaves (the right-most leaf wins a tie)
        self.e1, self.e2 = np.zeros((len(tris), 3), F), np.zeros((len(tris), 3), F)
        n = np.zeros(3, F)
        for k, t in enumerate(tris):
            orc.lib().orc_triangle_new(orc._fp(t[0:3].copy()), orc._fp(t[3:6].copy()), orc._fp(t[6:9].copy()),
                                       orc._fp(self.e1[k]), orc._fp(self.e2[k]), orc._fp(n))
            bmin, bmax = np.zeros(3, F), np.zeros(3, F)
            orc.lib().orc_triangle_bbox(orc._fp(t[0:3].copy()), orc._fp(t[3:6].copy()), orc._fp(t[6:9].copy()),
                                        orc._fp(bmin), orc._fp(bmax))
            assert np.array_equal(bmin, self.lo[k]) and np.array_equal(bmax, self.hi[k])
        self.pointers, self.kept = None, {}                 # candidates()
        self.rank = np.zeros(self.n, np.int64)
        self.rank[self.osc.leaf_order()] = np.arange(self.n)
        if not len(self.spheres):
            self.ref_rank = rtx.ref_leaf_rank(tris)
        self.leaf_of = np.zeros(self.n, np.int64)          # primitive -> record of its leaf in nodes()
        for i in np.nonzero(self.nodes[:, 7] & LEAF)[0]:
            first = int(self.nodes[i, 7]) & INDEX
            self.leaf_of[self.order[first:first + int(self.nodes[i, 3])]] = i

    def tables(self, orc):
        return ss.prim_tables(orc, self.tris, self.rgb, self.extra.get("spheres"), self.extra.get("sphere_rgb"))


def candidates(orc, b, o, d):
    """the reference's leaf rule for every primitive against one ray: {primitive: t} of those BVHNode::intersect would
    return from the primitive's leaf (bvh.rs:52-74); kept per scene and ray"""
    o, d = orc.f3(o), orc.f3(d)
    key = o.tobytes() + d.tobytes()
    if key in b.kept:
        return b.kept[key]
    if b.pointers is None:                             # per primitive: (v0 or centre, e1, e2, own box), contiguous rows
        first = np.ascontiguousarray(np.concatenate([b.tris[:, 0:3], b.spheres[:, :3]]))
        lo, hi = np.ascontiguousarray(b.lo), np.ascontiguousarray(b.hi)
        b.pointers = (first, lo, hi, [(orc._fp(first[k]), orc._fp(b.e1[k]) if k < len(b.tris) else None,
                                       orc._fp(b.e2[k]) if k < len(b.tris) else None, orc._fp(lo[k]), orc._fp(hi[k])) for k in range(b.n)])
    L, out = orc.lib(), {}
    po, pd = orc._fp(o), orc._fp(d)
    t, tb, af = C.c_float(), C.c_float(), C.c_int()
    pt, ptb = C.cast(C.byref(t), orc.f32p), C.cast(C.byref(tb), orc.f32p)
    for k, (first, e1, e2, lo, hi) in enumerate(b.pointers[3]):
        if e1 is not None:
            some = L.orc_triangle_intersect(first, e1, e2, po, pd, pt)
        else:
            some = L.orc_sphere_intersect(first, float(b.spheres[k - len(b.tris), 3]), po, pd, pt)
        if some and not t.value < 1.0 and L.orc_bbox_intersect(lo, hi, po, pd, ptb, C.byref(af)):
            out[k] = F(t.value)
    b.kept[key] = out
    return out


def box_entry(lo, hi, o, d, widen):
    """(passes, entry) of a ray into boxes widened by `widen`, float64: a superset of the kernel's multiply-based test;
    lo, hi: [..., 3]"""
    with np.errstate(divide="ignore", invalid="ignore"):
        a = (lo.astype(np.float64) - widen - o) / d
        c = (hi.astype(np.float64) + widen - o) / d
    near, far = np.minimum(a, c).max(axis=-1), np.maximum(a, c).min(axis=-1)
    return (near <= far) & (far >= 0.0), np.maximum(near, 0.0)


def emulate(b, stream, lanes, prune):
    """walk_stream for one wavefront.  lanes: [(origin, unit direction, candidates)] -> [(primitive or NO_HIT, t)] per lane"""
    n_nodes, n_global = len(stream), int(b.info["n_global"])
    lo, hi = stream[:, 0:3].view(F), stream[:, 4:7].view(F)
    best = [[NO_HIT, np.inf] for _ in lanes]
    # every lane against every record at once: [lane, record]
    tests = [box_entry(lo, hi, np.asarray(o, np.float64), np.asarray(d, np.float64), 2.0 * b.cull_delta) for o, d, _ in lanes]
    ok, entry = np.stack([t[0] for t in tests]), np.stack([t[1] for t in tests])

    def leaf(first, count):
        for k in b.order[first:first + count]:
            for lane, (_, _, cand) in enumerate(lanes):
                if int(k) in cand:
                    t, cur = cand[int(k)], best[lane]
                    if t < cur[1] or (t == cur[1] and cur[0] != NO_HIT and b.rank[k] > b.rank[cur[0]]):
                        best[lane] = [int(k), t]

    def somebody_passes(i):
        if not prune:
            return bool(ok[:, i].any())
        far = np.array([float(cur[1]) for cur in best]) * (1.0 + 2.0 ** -15)
        return bool((ok[:, i] & ~(entry[:, i] > far)).any())

    i = 1 if n_nodes > 1 else 0
    if n_global:
        leaf(0, n_global)
        i = 2
    while i < n_nodes:
        link, info = int(stream[i, 3]), int(stream[i, 7])
        passes = somebody_passes(i)
        if info & LEAF:
            if passes:
                leaf(info & INDEX, link)
            i += 1
        else:
            i = i + 1 if passes else link
    return [(k, F(t) if k != NO_HIT else F(0.0)) for k, t in best]


def verdicts(orc, b, stream, origins, units, exp, wave=1):
    """per ray: (unpruned emulation agrees with the oracle, exposed), the rays walked `wave` at a time in the given order"""
    agrees, exposed = np.zeros(len(origins), bool), np.zeros(len(origins), bool)
    for w0 in range(0, len(origins), wave):
        idx = range(w0, min(w0 + wave, len(origins)))
        lanes = [(origins[k], units[k], candidates(orc, b, origins[k], units[k])) for k in idx]
        plain, pruned = emulate(b, stream, lanes, False), emulate(b, stream, lanes, True)
        for k, p, q in zip(idx, plain, pruned):
            agrees[k] = p[0] == exp["prim"][k] and (p[0] == NO_HIT or p[1].tobytes() == exp["t"][k].tobytes())
            exposed[k] = agrees[k] and q[0] != p[0]
    return agrees, exposed


def prefilter(b, origins, units):
    """np_ref's vectorised float32 closest hit with the leaf's own box: only SELECTS rays worth the oracle's time (spheres are
    not in it; the emulation decides)"""
    _, t, prim = np_ref.closest_hit(np_ref.Tris(b.tris), origins, units)
    return prim, t


def scene(rtx, orc, samples, name):
    """name: 'triangles' or 'sphere' -> {order: Built}"""
    def make():
        tris, rgb, extra, groups = primitives(name == "sphere")
        mt, me = mirror(tris, extra)
        return dict(built=Built(rtx, orc, samples, tris, rgb, extra, groups),
                    mirrored=Built(rtx, orc, samples, mt, rgb, me, groups))
    return qs._once("prune_scene_" + name, make)


def _towards(b, prims, seed, n):
    rng = np.random.default_rng(seed)
    per = -(-n // len(prims))
    pts = np.concatenate([points_on(b.tris[k], rng, per) for k in prims])[:n]
    return np.zeros((n, 3), F), pts.astype(F)


def ray_sets(rtx, orc, samples, name):
    """-> dict(order: dict(set name: (origins, directions, expected records, units)), 'exposed_prim', 'counts').
    The rays are chosen on the order in which the emulation exposes them, and traced in both (mirrored with the scene)."""
    def make():
        sc = scene(rtx, orc, samples, name)
        b0 = sc["built"]
        target = int(b0.groups["behind"][0])
        # rays from the origin towards points of the first ill-conditioned triangle; np_ref picks those it answers with that
        # triangle nearer than the wall, the emulation (oracle candidates) confirms them one by one
        o, d = _towards(b0, [target], 11, N_DRAWS)
        units = ss.units_of(orc, d)
        prim, t = prefilter(b0, o, units)
        likely = np.nonzero((prim == target) & (t < 0.999 * (WALL_Z / units[:, 2])))[0]
        out = dict(exposed_prim=target, counts={}, likely=len(likely))
        chosen_order = chosen = None
        for order in ORDERS:
            b = sc[order]
            oo, dd = (o, d) if order == "built" else (mirrored_rays(o), mirrored_rays(d))
            exp, uu = qs.oracle_hits(orc, b.osc, oo[likely], dd[likely], qs.HIT_DTYPE)
            _, exposed = verdicts(orc, b, b.nodes, oo[likely], uu, exp)
            out["counts"][order] = int(exposed.sum())
            if chosen is None and exposed.sum() >= N_EXPOSED:
                chosen_order, chosen = order, likely[exposed][:N_EXPOSED]
        out["chosen_order"] = chosen_order
        if chosen is None:
            return out
        ordinary_o = np.zeros((1000, 3), F)
        g = np.random.default_rng(12)
        ordinary_d = np.stack([g.uniform(-190.0, 190.0, 1000), g.uniform(-190.0, 190.0, 1000), np.full(1000, WALL_Z)], axis=1).astype(F)
        place = np.sort(np.random.default_rng(13).choice(1000 + N_EXPOSED, N_EXPOSED, replace=False))
        mixed_o, mixed_d = np.zeros((1000 + N_EXPOSED, 3), F), np.zeros((1000 + N_EXPOSED, 3), F)
        rest = np.setdiff1d(np.arange(1000 + N_EXPOSED), place)
        mixed_d[place], mixed_d[rest] = d[chosen], ordinary_d
        # towards the triangles in front of the wall: of 4,000 drawn rays the (few) ones np_ref answers with such a triangle
        # BEHIND the wall, at most 32, and the first 64 of the others
        fo, fd = _towards(b0, b0.groups["front"], 21, 4000)
        fu = ss.units_of(orc, fd)
        front_t = np_ref.closest_hit(np_ref.Tris(b0.tris[b0.groups["front"]]), fo, fu)[1]
        late = np.nonzero(np.isfinite(front_t) & (front_t > np.abs(WALL_Z / fu[:, 2])))[0][:32]
        pick = np.concatenate([late, np.setdiff1d(np.arange(4000), late)[:64]])
        controls = dict(front=(fo[pick], fd[pick]), well=_towards(b0, b0.groups["well"], 22, 64))
        if name == "sphere":
            c = np.asarray(SPHERE_BEHIND[:3])
            u = np.random.default_rng(23).normal(size=(64, 3))
            u /= np.linalg.norm(u, axis=1)[:, None]
            controls["sphere"] = (np.zeros((64, 3), F), (c + 0.8 * SPHERE_BEHIND[3] * u).astype(F))
        for order in ORDERS:
            b = sc[order]
            turn = (lambda v: v) if order == "built" else mirrored_rays
            sets = {}
            for key, (so, sd) in dict(exposed=(o[chosen], d[chosen]), mixed=(mixed_o, mixed_d), ordinary=(ordinary_o, ordinary_d),
                                      **controls).items():
                so, sd = turn(so), turn(sd)
                exp, uu = qs.oracle_hits(orc, b.osc, so, sd, qs.HIT_DTYPE)
                sets[key] = (so, sd, exp, uu)
            out[order] = sets
        out["place"] = place
        return out
    return qs._once("prune_rays_" + name, make)


def checked(rtx, orc, samples, name, order, key, wave=1):
    """verdicts() of one ray set on the ray-batch kernels' stream, `wave` rays to a wavefront in the set's order: built once"""
    def make():
        b = scene(rtx, orc, samples, name)[order]
        o, _, exp, units = ray_sets(rtx, orc, samples, name)[order][key]
        return verdicts(orc, b, b.nodes, o, units, exp, wave)
    return qs._once("prune_checked_%s_%s_%s_%d" % (name, order, key, wave), make)


def occlusion_targets(origins, directions):
    """targets beyond the wall along the same rays: where the ray meets z = +-300"""
    d = directions.astype(np.float64)
    return (origins + d * (300.0 / np.abs(d[:, 2:3]))).astype(F)


def occlusion_set(orc, b, origins, directions):
    t = occlusion_targets(origins, directions)
    return qs.pair_sets(orc, b.osc, origins, t)["occlusion"]


def without(orc, b, prim):
    """the oracle's scene with one triangle taken far away (the primitive numbers stay): what a walk that never tests that
    triangle answers"""
    tris = b.tris.copy()
    tris[prim] = (0.0, -5000.0, 0.0, 1.0, -5000.0, 0.0, 0.0, -5000.0, 1.0)
    return orc.Scene(b.args[0], b.args[1], tris, b.rgb, b.args[4], **b.kw)


def shade_batch(orc, b, samples, s, osc=None):
    """rtx_shade_rays' expected records for a ray set at nb_ray = 1: render_pixel composed from oracle pieces"""
    o, d = s[0], s[1]
    return ss.shade_set(orc, osc or b.osc, o, d, 1, NB_LIGHT, b.kw["light_tri"], samples, b.tables(orc))


# ---------------------------------------------------------------------------------------------------------- 1 x 1 frames
def primary_ray(orc, w, h, px, py, eye, look_at, up, distance, samples):
    """create_rays' ray 0 of pixel (px, py) by the oracle (main.rs:151-178)"""
    u, v, ww = (np.zeros(3, F) for _ in range(3))
    orc.lib().orc_camera_new(orc._fp(orc.f3(eye)), orc._fp(orc.f3(look_at)), orc._fp(orc.f3(up)), orc._fp(u), orc._fp(v), orc._fp(ww))
    o, d = np.zeros(3, F), np.zeros(3, F)
    s = np.ascontiguousarray(samples, F)
    orc.lib().orc_create_ray(px, py, 0, w, h, orc._fp(orc.f3(eye)), orc._fp(u), orc._fp(v), orc._fp(ww), float(distance),
                             orc._fp(s), len(s), orc._fp(o), orc._fp(d))
    return o, d


def frame(rtx, orc, samples, name, order):
    """A 1 x 1 frame whose one primary ray is exposed: eye at the origin, looking at a point of the first ill-conditioned
    triangle; the first point of a seeded draw for which the emulation, on the primary rays' stream of a scene created with
    that camera, says so.  `samples` is a constant table: the ray goes through the frame's centre, along -w.
    -> dict(b = Built with that camera, camera, ray (o, unit d), exp, exposed, tried)"""
    def make():
        sc = scene(rtx, orc, samples, name)[order]
        target = int(sc.groups["behind"][0])
        pts = points_on(sc.tris[target], np.random.default_rng(31), 400).astype(F)
        rays = [primary_ray(orc, 1, 1, 0, 0, EYE, p, (0.0, 1.0, 0.0), FRAME_DISTANCE, samples) for p in pts]
        units = np.stack([r[1] for r in rays])
        prim, t = prefilter(sc, np.zeros_like(units), units)
        likely = np.nonzero((prim == target) & (t < 0.999 * np.abs(WALL_Z / units[:, 2])))[0]
        for tried, k in enumerate(likely):
            # the light on the eye's side of the wall: the point in front of the wall and the wall's own point are both lit,
            # in different colours (the primary rays' stream does not depend on the light)
            z = -20.0 * float(np.sign(sc.tris[0, 2]))
            camera = dict(eye=EYE, look_at=tuple(float(x) for x in pts[k]), up=(0.0, 1.0, 0.0), distance=FRAME_DISTANCE,
                          light_tri=(-10.0, 40.0, z, 10.0, 40.0, z, 0.0, 55.0, z + 5.0))
            b = Built(rtx, orc, samples, sc.tris, sc.rgb, sc.extra, sc.groups, camera=camera, frame=(1, 1))
            o, d = rays[k]
            exp = np.zeros(1, qs.HIT_DTYPE)                  # (d is Ray::new's already: not normalised a second time)
            exp["prim"] = NO_HIT
            h = b.osc.closest_hit(o, d)
            if h.hit:
                exp["prim"][0], exp["t"][0], exp["p_hit"][0] = h.tri, h.t, list(h.p_hit)
            agrees, exposed = verdicts(orc, b, b.primary, o[None], d[None], exp)
            if exposed[0]:
                ref, stats = b.osc.render_rows(mode=orc.MODE_BVH)
                # rtx_render_view walks the library's own stream, which the light orders: the same view of the ray sets' scene
                # (the light behind everything), where the pixel may be black either way and the hit record decides
                seen = dict(camera, light_tri=LIGHT_TRI)
                bv = Built(rtx, orc, samples, sc.tris, sc.rgb, sc.extra, sc.groups, camera=seen, frame=(1, 1))
                on_nodes = bool(verdicts(orc, bv, bv.nodes, o[None], d[None], exp)[1][0])
                return dict(b=b, camera=camera, ray=(o, d), exp=exp, exposed=True, exposed_on_nodes=on_nodes, tried=tried + 1,
                            target=target, ref=ref, seen=bv, seen_ref=bv.osc.render_rows(mode=orc.MODE_BVH)[0],
                            stats=stats, without=without(orc, b, target).render_rows(mode=orc.MODE_BVH)[0])
        return dict(exposed=False, tried=len(likely))
    return qs._once("prune_frame_%s_%s" % (name, order), make)
