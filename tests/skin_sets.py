"""Fixtures for the rtx_scene_pose_skinned tests — a pose whose triangle corners blend up to four moves by the weights of
a skin bound to the scene once — with the CPU oracle's answers: numpy, the oracle binding and the library's host side
only, no GPU.

Built on prims_sets' "yard" (46 primitives, a 24 x 16 frame, 2 rays per pixel, 10 light samples), on its count scenes
(255, 256 and 257 primitives, every third a sphere) and on triangle scenes of 21, 22, 85 and 86 triangles (63, 66, 255 and
258 corners: a wavefront's and a workgroup's edge).  A fixture is two dicts: skin(rtx, name), the keywords of
rtx.Scene.skin (bones [n_tris, 3, 4], weights [n_tris, 3, 4], sphere_bone [n_spheres] or None), and moves(rtx, name), the
keywords of rtx.Scene.pose_skinned (moves [n, 12], radius_scale [n] or None, rgb, sphere_rgb).  Expected values ALWAYS come
from an oracle scene CREATED WITH rtx_scene_skinned_prims' OUTPUT (stated), as moves_sets does it; restated() is the same
statement in numpy, one np.float32 operation per product and sum, which tests/test_skin_sets.py holds the library's
against.  Everything is built once per process (query_sets._once)."""
import contextlib

import numpy as np

import moves_sets as mv
import prims_sets as pm
import query_sets as qs
import shade_sets as ss
from query_sets import F

NONE = mv.NONE
POSES = ("bend", "one", "four", "lean", "rest", "balls", "all")
CHANGING = ("bend", "one", "four", "lean", "balls", "all")
CALLS = ("bend", "four", "balls", "all")          # the poses every posed call is run over
BEND_DEGREES = 70.0
# `one`'s second move, followed by the ground alone: x and z as they are, y pressed to -0.0 where every product is -0.0 —
# the ground's third corner (+0.0, +0.0, 10000): a moved pose keeps that -0.0, a skinned one adds 0 * rest to it: +0.0
PRESS = np.array([1, 0, 0, 0, -0.0, -0.0, -0.0, -0.0, 0, 0, 1, 0], F)


def heights(rtx):
    """per corner of the yard's triangles [41, 3]: 0 at the cluster's lowest vertex, 1 at its highest, as f32 — a function
    of the corner's rest words alone"""
    y = pm.yard(rtx)["tris"].reshape(-1, 3, 3)[:, :, 1]
    cluster = np.delete(y, pm.GROUND_NUMBER, axis=0)
    lo, hi = F(cluster.min()), F(cluster.max())
    return ((y - lo) / F(hi - lo)).astype(F)


def bend_moves(rtx):
    """the two moves of `bend`: the foot stays (identity), the head turns about the vertical and shifts"""
    c = mv.cluster_centre(rtx)
    a = np.deg2rad(BEND_DEGREES)
    head = mv.about([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]], c)
    head[3] = F(head[3] + F(6.0))
    return np.stack([mv.IDENTITY, head]).astype(F)


def four_moves(rtx):
    c = mv.cluster_centre(rtx)
    turn = lambda d: [[np.cos(np.deg2rad(d)), 0, np.sin(np.deg2rad(d))], [0, 1, 0], [-np.sin(np.deg2rad(d)), 0, np.cos(np.deg2rad(d))]]
    return np.stack([mv.about(turn(20.0), c), mv.about(turn(-30.0), c), mv.translation((4.0, 3.0, -2.0)),
                     mv.about([[1.1, 0.3, 0], [0, 1.05, 0], [0.1, 0, 0.9]], c)]).astype(F)


def skin(rtx, name):
    """keywords of rtx.Scene.skin for the fixture"""
    n = pm.N_MESH + 1
    bones = np.full((n, 3, 4), NONE, np.uint32)
    weights = np.zeros((n, 3, 4), F)
    sphere_bone = None
    cluster = np.ones(n, bool)
    cluster[pm.GROUND_NUMBER] = False
    if name in ("bend", "all"):
        h = heights(rtx)
        bones[cluster, :, 0], bones[cluster, :, 1] = 0, 1
        weights[:, :, 0], weights[:, :, 1] = (F(1.0) - h).astype(F), h
        weights[pm.GROUND_NUMBER] = 0.0
        if name == "all":
            sphere_bone = (2 + np.arange(pm.N_SPHERES)).astype(np.uint32)
    elif name == "one":
        bones[cluster, :, 0] = 0
        bones[pm.GROUND_NUMBER, :, 0] = 1
        weights[:, :, 0] = 1.0
    elif name == "four":
        bones[cluster] = np.arange(4, dtype=np.uint32)
        k = np.arange(3 * n, dtype=np.float64).reshape(n, 3, 1)
        weights[:] = (np.array([0.4, 0.3, 0.2, 0.25]) * (1.0 + 0.003 * k)).astype(F)         # (1.15 and more: no partition of one)
    elif name == "lean":
        bones[cluster, :, 0] = 0
        weights[:, :, 0], weights[:, :, 1] = 0.6, 0.4                                        # the second slot is NONE: the rest position
    elif name == "rest":
        weights[:] = 0.25
    elif name == "balls":
        weights[:, :, 0] = 1.0
        sphere_bone = np.arange(pm.N_SPHERES, dtype=np.uint32)
    else:
        raise KeyError(name)
    return dict(bones=bones, weights=weights, sphere_bone=sphere_bone)


def moves(rtx, name):
    """keywords of rtx.Scene.pose_skinned / skinned_prims for the fixture (rgb and sphere_rgb: pose_skinned only)"""
    kw = dict(moves=None, radius_scale=None, rgb=None, sphere_rgb=None)
    if name == "bend":
        kw["moves"] = bend_moves(rtx)
    elif name == "one":
        kw["moves"] = np.stack([mv.turn_move(rtx), PRESS])
    elif name == "four":
        kw["moves"] = four_moves(rtx)
    elif name in ("lean", "rest"):
        kw["moves"] = mv.turn_move(rtx).reshape(1, 12)
    elif name == "balls":
        kw["moves"], kw["radius_scale"] = mv.ball_moves()
    elif name == "all":
        balls, scale = mv.ball_moves()
        kw["moves"] = np.concatenate([bend_moves(rtx), balls])
        kw["radius_scale"] = np.concatenate([np.array([3.0, 3.0], F), scale])                # (no sphere follows moves 0 and 1)
        y = pm.yard(rtx)
        kw["rgb"], kw["sphere_rgb"] = pm.recoloured(y["rgb"], y["sphere_rgb"])
    else:
        raise KeyError(name)
    kw["moves"] = np.ascontiguousarray(kw["moves"], F)
    return kw


def statement_kw(kw):
    return {k: kw[k] for k in ("moves", "radius_scale")}


def one_as_groups():
    """`one`'s skin as a moved pose's group array: the cluster follows move 0, the ground move 1"""
    g = np.full(pm.N_PRIMS, NONE, np.uint32)
    g[mv.cluster_at()] = 0
    g[pm.GROUND_AT] = 1
    return g


def _point(m, p):
    out = np.zeros(3, F)
    for r in range(3):
        a = F(m[4 * r] * p[0])
        b = F(m[4 * r + 1] * p[1])
        c = F(m[4 * r + 2] * p[2])
        out[r] = F(F(F(a + b) + c) + m[4 * r + 3])
    return out


def restated(tris, spheres, bones, weights, sphere_bone, moves, radius_scale=None, form="stated"):
    """skin_statement in numpy: every product and every sum a separate np.float32 operation, in the stated order.
    form = "pairwise": (a + b) + (c + d) instead; "fused": every sum takes its product unrounded (the products and sums
    in double, rounded to f32 after each SUM: what a contracted multiply-add gives, since the product of two f32 is exact
    in double and one rounding follows) — the two evaluations a kernel must NOT be"""
    tris, spheres = np.array(tris, F).reshape(-1, 3, 3), np.array(spheres, F).reshape(-1, 4)
    m = np.asarray(moves, F).reshape(-1, 12)
    bones = np.asarray(bones, np.uint32).reshape(-1, 3, 4)
    weights = np.asarray(weights, F).reshape(-1, 3, 4)
    D = np.float64
    with np.errstate(all="ignore"):
        for t in range(len(tris)):
            for c in range(3):
                b, w, p = bones[t, c], weights[t, c], tris[t, c].copy()
                if (b >= len(m)).all():
                    continue
                q = [(_point(m[int(b[k])], p) if b[k] < len(m) else p) for k in range(4)]
                for r in range(3):
                    if form == "fused":
                        acc = F(D(w[0]) * D(q[0][r]))
                        for k in (1, 2, 3):
                            acc = F(D(acc) + D(w[k]) * D(q[k][r]))
                        tris[t, c, r] = acc
                        continue
                    x = [F(w[k] * q[k][r]) for k in range(4)]
                    tris[t, c, r] = F(F(x[0] + x[1]) + F(x[2] + x[3])) if form == "pairwise" else F(F(F(x[0] + x[1]) + x[2]) + x[3])
        for s in range(len(spheres)):
            g = NONE if sphere_bone is None else int(sphere_bone[s])
            if g < len(m):
                spheres[s, :3] = _point(m[g], spheres[s, :3].copy())
                if radius_scale is not None:
                    spheres[s, 3] = F(spheres[s, 3] * F(radius_scale[g]))
    return tris.reshape(-1, 9), spheres


@contextlib.contextmanager
def open_skinned(rtx, samples, name, **kw):
    """the library's scene of the yard with the fixture's skin bound"""
    with pm.open_yard(rtx, samples, **kw) as scene:
        scene.skin(**skin(rtx, name))
        yield scene


def stated(rtx, samples, name):
    """the posed primitives as rtx_scene_skinned_prims states them, every array in full: dict(tris, rgb, spheres, sphere_rgb)"""
    def make():
        kw = moves(rtx, name)
        y = pm.yard(rtx)
        with open_skinned(rtx, samples, name) as scene:
            v, sph = scene.skinned_prims(**statement_kw(kw))
        out = dict(tris=v, spheres=sph, rgb=(y["rgb"] if kw["rgb"] is None else kw["rgb"]).copy(),
                   sphere_rgb=(y["sphere_rgb"] if kw["sphere_rgb"] is None else kw["sphere_rgb"]).copy())
        out = {k: np.ascontiguousarray(a, F) for k, a in out.items()}
        for a in out.values():
            a.setflags(write=False)
        return out
    return qs._once("skin_stated_" + name, make)


def given(rtx, samples, name):
    """keywords of rtx.Scene.pose_prims for the arrays the statement gives: the pose a skinned pose must equal"""
    return pm.pose_kw(stated(rtx, samples, name))


def posed(orc, rtx, samples, name):
    """prims_sets.render of the oracle scene created with the stated primitives"""
    def make():
        prims = stated(rtx, samples, name)
        return dict(pm.render(orc, samples, prims), prims=prims)
    return qs._once("skin_posed_" + name, make)


def lit_frame(orc, rtx, samples, name):
    def make():
        tri, count = pm.POSE_LIGHT
        r = pm.render(orc, samples, stated(rtx, samples, name), light_tri=tri, nb_light_sample=count)
        r["osc"].close()
        return r["frame"], r["stats"]
    return qs._once("skin_lit_" + name, make)


def tables(orc, rtx, samples, name):
    def make():
        p = stated(rtx, samples, name)
        return ss.prim_tables(orc, p["tris"], p["rgb"], p["spheres"], p["sphere_rgb"], pm.kinds())
    return qs._once("skin_tables_" + name, make)


def composition(orc, rtx, samples, name):
    """render_pixel composed from oracle pieces on the posed oracle scene for the yard view's rays"""
    def make():
        o, d = mv.view_rays(orc, samples)
        return ss.shade_set(orc, posed(orc, rtx, samples, name)["osc"], o, d, pm.NB_RAY, pm.NB_LIGHT, orc.LIGHT_TRI, samples[:4096],
                            tables(orc, rtx, samples, name))
    return qs._once("skin_comp_" + name, make)


def query_set(orc, rtx, samples, name, n=200):
    """moves_sets.query_set's rays and point pairs, answered on this pose's oracle scene"""
    def make():
        osc = posed(orc, rtx, samples, name)["osc"]
        rng = np.random.default_rng(31)
        o = rng.uniform((-120.0, 5.0, -80.0), (120.0, 150.0, 200.0), size=(n, 3)).astype(F)
        aim = rng.uniform((-100.0, 0.0, -60.0), (100.0, 40.0, 120.0), size=(n, 3)).astype(F)
        d = (aim - o).astype(F)
        exp, _ = qs.oracle_hits(orc, osc, o, d, qs.HIT_DTYPE)
        t = (o + d * rng.uniform(0.3, 1.6, size=(n, 1)).astype(F)).astype(F)
        texp, _ = qs.oracle_hits(orc, osc, o, (t - o).astype(F), qs.HIT_DTYPE)
        return (o, d, exp), (o, t, texp, qs.expected_occlusion(texp, o, t))
    return qs._once("skin_query_" + name, make)


def hard_rays(orc, rtx, samples):
    """33 rays straight down onto the bent cluster, each with a -0.0 component, answered by the own tree of the oracle
    scene created with `bend`'s primitives, and the answers of their +0.0 twins"""
    def make():
        osc = posed(orc, rtx, samples, "bend")["osc"]
        c = mv.cluster_centre(rtx)
        rng = np.random.default_rng(12)
        o = (c + np.concatenate([rng.uniform(-25.0, 25.0, (33, 1)), np.full((33, 1), 90.0), rng.uniform(-25.0, 25.0, (33, 1))],
                                axis=1)).astype(F)
        d = np.tile(np.array([-0.0, -1.0, 0.125], F), (33, 1))
        d[::3, 2] = -0.0
        d[::3, 0] = 0.0625
        exp, _ = qs.oracle_hits(orc, osc, o, d, qs.HIT_DTYPE)
        twin, _ = qs.oracle_hits(orc, osc, o, np.where(d == 0, F(0.0), d).astype(F), qs.HIT_DTYPE)
        return o, d, exp, twin
    return qs._once("skin_hard", make)


def ribbon():
    """a mesh whose triangles SHARE corners, for the crack test: a column of 8 quads, two triangles each -> (tris [16, 9],
    skin keywords with `bend`'s kind of weights: by the corner's own height, bones 0 and 1)"""
    rows = np.array([[[-3.0 + 0.37 * k, 5.0 * k, 1.0 + 0.21 * k], [4.0 - 0.29 * k, 5.0 * k, 2.0 - 0.13 * k]] for k in range(9)], F)
    tris = []
    for k in range(8):
        a, b, c, d = rows[k, 0], rows[k, 1], rows[k + 1, 0], rows[k + 1, 1]
        tris += [np.concatenate([a, b, c]), np.concatenate([b, d, c])]
    tris = np.ascontiguousarray(np.stack(tris), F)
    h = (tris.reshape(-1, 3, 3)[:, :, 1] / F(40.0)).astype(F)
    bones = np.full((16, 3, 4), NONE, np.uint32)
    bones[:, :, 0], bones[:, :, 1] = 0, 1
    weights = np.zeros((16, 3, 4), F)
    weights[:, :, 0], weights[:, :, 1] = (F(1.0) - h).astype(F), h
    return tris, dict(bones=bones, weights=weights, sphere_bone=None)


# the exact sphere-triangle tie of prims_sets, reached by a skin: the sphere follows a translation of (-5, 0, 0) and every
# corner of the two triangles is NONE
TIE_SKIN = dict(bones=np.full((2, 3, 4), NONE, np.uint32), weights=np.zeros((2, 3, 4), F), sphere_bone=np.array([0], np.uint32))
TIE_MOVES = dict(moves=mv.translation((-5.0, 0.0, 0.0)).reshape(1, 12), radius_scale=None)

# a triangle holding a -0.0 (and one that does not), for `rest` and for the sign of a zero
ZERO_TRIS = np.array([[-0.0, 1.0, 2.0, 3.0, -0.0, 1.0, 2.0, 5.0, -0.0], [1.0, 1.0, 1.0, 4.0, 1.0, 1.0, 1.0, 6.0, 2.0]], F)


def open_zero(rtx, samples):
    return rtx.Scene(8, 8, ZERO_TRIS, np.ones((2, 3), F), samples[:4096], nb_light_sample=4, reference_tree=rtx.REFTREE_NEVER,
                     tie_rank=None)


# ---- the count scenes (prims_sets.size_scenes' 255 / 256 / 257 primitives, every third a sphere) and the smallest ones
COUNTS = mv.COUNTS
SMALLEST = (21, 22, 85, 86)             # triangles: 63 / 66 corners (a wavefront's edge), 255 / 258 (a workgroup's)


def dealt_skin(n_tris, n_spheres, n_moves, seed):
    """bones dealt by corner number over n_moves, every fifth corner's third slot NONE, every seventh corner all NONE;
    weights a partition of one (so a blend of in-range points stays in range); spheres dealt by number, every fourth NONE"""
    rng = np.random.default_rng(seed)
    c = np.arange(3 * n_tris).reshape(n_tris, 3, 1)
    bones = ((c + np.arange(4)) % n_moves).astype(np.uint32)
    bones[:, :, 2] = np.where(c[:, :, 0] % 5 == 4, NONE, bones[:, :, 2])
    bones[(c[:, :, 0] % 7 == 3)] = NONE
    w = rng.uniform(0.05, 1.0, (n_tris, 3, 4))
    weights = (w / w.sum(axis=2, keepdims=True)).astype(F)
    s = np.arange(n_spheres)
    sphere_bone = np.where(s % 4 == 3, NONE, s % n_moves).astype(np.uint32)
    return dict(bones=bones, weights=weights, sphere_bone=sphere_bone)


def count_cases(rtx):
    """(name, scene dict, skin keywords, moves keywords): the three count scenes under moves_sets' four dealt moves, and
    `many` on the 257: a move per primitive number, 257 of them"""
    sizes = pm.size_scenes(rtx)
    out = []
    for n in COUNTS:
        sc = sizes[n]
        m = mv.count_moves(len(sc["kinds"]))
        out.append((n, sc, dealt_skin(len(sc["tris"]), len(sc["spheres"]), 4, 5), dict(moves=m["moves"], radius_scale=m["radius_scale"])))
    sc = sizes["mixed257"]
    m = mv.count_moves(257, many=True)
    out.append(("many", sc, dealt_skin(len(sc["tris"]), len(sc["spheres"]), 257, 6), dict(moves=m["moves"], radius_scale=None)))
    return out


def smallest_cases(rtx):
    """(name, triangles [n, 9], skin keywords, moves keywords) of the triangle-only scenes: three maps that draw the mesh
    towards its box centre, so that every blend stays inside the scene's bound"""
    out = []
    for n in SMALLEST:
        tris = np.ascontiguousarray(rtx.synthetic_mesh(n), F)
        pts = tris.reshape(-1, 3).astype(np.float64)
        c = 0.5 * (pts.min(axis=0) + pts.max(axis=0))
        a = np.deg2rad(25.0)
        m = np.stack([mv.about(np.diag([0.5, 0.6, 0.7]), c), mv.about(0.6 * np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]]), c),
                      mv.about(np.diag([0.9, -0.4, 0.8]), c)]).astype(F)
        out.append(("tris%d" % n, tris, dealt_skin(n, 0, 3, 10 + n), dict(moves=m, radius_scale=None)))
    return out


def open_tris(rtx, samples, tris):
    return rtx.Scene(8, 8, tris, np.ones((len(tris), 3), F), samples[:4096], nb_light_sample=4, reference_tree=rtx.REFTREE_NEVER,
                     tie_rank=None)
