"""Fixtures for the rtx_scene_pose_moved tests — a pose whose vertices and spheres the device makes from the scene's
geometry as created and a small set of affine maps — with the CPU oracle's answers: numpy, the oracle binding and the
library's host side only, no GPU.

Built on prims_sets' "yard" (46 primitives, a 24 x 16 frame, 2 rays per pixel, 10 light samples) and on its count scenes
(255, 256 and 257 primitives, every third a sphere).  A pose here is the keywords of rtx.Scene.pose_moved: moves [n, 12],
group [n_prims] or None, radius_scale [n] or None, rgb, sphere_rgb.  Its expected values ALWAYS come from an oracle scene
CREATED WITH rtx_scene_moved_prims' OUTPUT (stated), as prims_sets.oracle_scene does it; restated() is the same statement
in numpy, one np.float32 operation per product and sum, which tests/test_moves_sets.py holds the library's against.
Everything is built once per process (query_sets._once)."""
import numpy as np

import prims_sets as pm
import query_sets as qs
import shade_sets as ss
from query_sets import F

NONE = 0xFFFFFFFF
POSES = ("turn", "balls", "shear", "all", "same", "unit")
CHANGING = ("turn", "balls", "shear", "all")
TURN_DEGREES = 40.0
IDENTITY = np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], F)
SPHERE_AT = np.asarray(pm.SPHERE_AT)


def cluster_at():
    """Vec positions of the cluster's triangles (every triangle but the ground)"""
    k = pm.kinds()
    return np.array([i for i in range(pm.N_PRIMS) if k[i] == 0 and i != pm.GROUND_AT])


def cluster_centre(rtx):
    t = pm.yard(rtx)["tris"].astype(np.float64).reshape(-1, 3, 3)
    pts = np.delete(t, pm.GROUND_NUMBER, axis=0).reshape(-1, 3)
    return 0.5 * (pts.min(axis=0) + pts.max(axis=0))


def about(linear, centre):
    """the 3 x 4 map p -> centre + linear (p - centre), composed in double and rounded to f32 once"""
    linear = np.asarray(linear, np.float64)
    return np.concatenate([linear, (centre - linear @ centre).reshape(3, 1)], axis=1).reshape(12).astype(F)


def turn_move(rtx, degrees=TURN_DEGREES):
    """`degrees` about the vertical through the cluster's box centre (prims_sets.turned's sense)"""
    a = np.deg2rad(degrees)
    return about([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]], cluster_centre(rtx))


def translation(t):
    m = IDENTITY.copy()
    m[[3, 7, 11]] = t
    return m


def ball_moves():
    """a move per sphere, and their radius factors: two change place, one rolls in front of the cluster, one goes to other
    ground and doubles (lifted by its radius, so it stays on the ground), one shrinks to radius 0"""
    s = pm.SPHERES.astype(np.float64)
    t = np.zeros((5, 3))
    t[0], t[1] = s[1, :3] - s[0, :3], s[0, :3] - s[1, :3]
    t[0, 1] = t[1, 1] = 0.0
    t[2] = np.array([2.0, 20.0, 40.0]) - s[2, :3]
    t[3] = np.array([88.0, 2.0 * s[3, 3], 20.0]) - s[3, :3]
    return np.stack([translation(x) for x in t]).astype(F), np.array([1, 1, 1, 2, 0], F)


def moves(rtx, name):
    """keywords of rtx.Scene.pose_moved / moved_prims for the pose (rgb and sphere_rgb: pose_moved only)"""
    group = np.full(pm.N_PRIMS, NONE, np.uint32)
    kw = dict(moves=None, group=group, radius_scale=None, rgb=None, sphere_rgb=None)
    if name == "turn":
        kw["moves"] = turn_move(rtx).reshape(1, 12)
        group[cluster_at()] = 0
    elif name == "balls":
        kw["moves"], kw["radius_scale"] = ball_moves()
        group[SPHERE_AT] = np.arange(5)
    elif name == "shear":       # two non-rigid maps, given to the cluster's triangles by the parity of their Vec position
        c = cluster_centre(rtx)
        kw["moves"] = np.stack([about([[1.2, 0.3, 0], [0, 1.2, 0], [0, 0, 1.2]], c), about([[1.2, -0.3, 0], [0, 1.2, 0], [0, 0, 1.2]], c)])
        at = cluster_at()
        group[at] = at % 2
    elif name == "all":
        balls, scale = ball_moves()
        kw["moves"] = np.concatenate([turn_move(rtx).reshape(1, 12), balls])
        kw["radius_scale"] = np.concatenate([np.array([3.0], F), scale])        # (no sphere follows move 0)
        group[cluster_at()] = 0
        group[SPHERE_AT] = 1 + np.arange(5)
        y = pm.yard(rtx)
        kw["rgb"], kw["sphere_rgb"] = pm.recoloured(y["rgb"], y["sphere_rgb"])
    elif name == "same":        # every group is NONE: the maps are followed by nobody
        kw["moves"] = np.stack([turn_move(rtx), translation((5.0, 6.0, 7.0))])
        kw["radius_scale"] = np.array([2.0, 0.5], F)
    elif name == "unit":        # the identity matrix on everything but the ground
        kw["moves"] = IDENTITY.reshape(1, 12).copy()
        group[:] = 0
        group[pm.GROUND_AT] = NONE
    else:
        raise KeyError(name)
    kw["moves"] = np.ascontiguousarray(kw["moves"], F)
    return kw


def statement_kw(kw):
    return {k: kw[k] for k in ("moves", "group", "radius_scale")}


def restated(tris, spheres, kinds, moves, group=None, radius_scale=None):
    """move_statement in numpy: every product and every sum a separate np.float32 operation, in the stated order"""
    tris, spheres = np.array(tris, F).reshape(-1, 3, 3), np.array(spheres, F).reshape(-1, 4)
    m = np.asarray(moves, F).reshape(-1, 12)
    kinds = np.asarray(kinds)
    group = np.zeros(len(kinds), np.uint32) if group is None else np.asarray(group, np.uint32)

    def point(mv, p):
        out = np.zeros(3, F)
        for r in range(3):
            a = F(mv[4 * r] * p[0])
            b = F(mv[4 * r + 1] * p[1])
            c = F(mv[4 * r + 2] * p[2])
            out[r] = F(F(F(a + b) + c) + mv[4 * r + 3])
        return out

    with np.errstate(all="ignore"):
        for n, at in enumerate(np.nonzero(kinds == 0)[0]):
            g = int(group[at])
            if g < len(m):
                for k in range(3):
                    tris[n, k] = point(m[g], tris[n, k].copy())
        for n, at in enumerate(np.nonzero(kinds != 0)[0]):
            g = int(group[at])
            if g < len(m):
                spheres[n, :3] = point(m[g], spheres[n, :3].copy())
                if radius_scale is not None:
                    spheres[n, 3] = F(spheres[n, 3] * F(radius_scale[g]))
    return tris.reshape(-1, 9), spheres


def stated(rtx, samples, name):
    """the posed primitives as rtx_scene_moved_prims states them, every array in full: dict(tris, rgb, spheres, sphere_rgb)"""
    def make():
        kw = moves(rtx, name)
        y = pm.yard(rtx)
        with pm.open_yard(rtx, samples) as scene:
            v, sph = scene.moved_prims(**statement_kw(kw))
        out = dict(tris=v, spheres=sph, rgb=(y["rgb"] if kw["rgb"] is None else kw["rgb"]).copy(),
                   sphere_rgb=(y["sphere_rgb"] if kw["sphere_rgb"] is None else kw["sphere_rgb"]).copy())
        out = {k: np.ascontiguousarray(a, F) for k, a in out.items()}
        for a in out.values():
            a.setflags(write=False)
        return out
    return qs._once("moves_stated_" + name, make)


def given(rtx, samples, name):
    """keywords of rtx.Scene.pose_prims for the arrays the statement gives: the pose a moved pose must equal"""
    return pm.pose_kw(stated(rtx, samples, name))


def posed(orc, rtx, samples, name):
    """prims_sets.render of the oracle scene created with the stated primitives"""
    def make():
        prims = stated(rtx, samples, name)
        return dict(pm.render(orc, samples, prims), prims=prims)
    return qs._once("moves_posed_" + name, make)


def lit_frame(orc, rtx, samples, name):
    def make():
        tri, count = pm.POSE_LIGHT
        r = pm.render(orc, samples, stated(rtx, samples, name), light_tri=tri, nb_light_sample=count)
        r["osc"].close()
        return r["frame"], r["stats"]
    return qs._once("moves_lit_" + name, make)


def tables(orc, rtx, samples, name):
    def make():
        p = stated(rtx, samples, name)
        return ss.prim_tables(orc, p["tris"], p["rgb"], p["spheres"], p["sphere_rgb"], pm.kinds())
    return qs._once("moves_tables_" + name, make)


def view_rays(orc, samples):
    """the yard view's rays: (origins, directions)"""
    (w, h), eye, look_at, distance = pm.YARD_VIEW
    import view_sets as vs
    o, d, _, _, _ = ss.camera_raw_rays(orc, w, h, eye, look_at, vs.UP, distance, samples[:4096], pm.NB_RAY)
    return o, d


def composition(orc, rtx, samples, name):
    """render_pixel composed from oracle pieces on the posed oracle scene for the yard view's rays"""
    def make():
        o, d = view_rays(orc, samples)
        return ss.shade_set(orc, posed(orc, rtx, samples, name)["osc"], o, d, pm.NB_RAY, pm.NB_LIGHT, orc.LIGHT_TRI, samples[:4096],
                            tables(orc, rtx, samples, name))
    return qs._once("moves_comp_" + name, make)


def query_set(orc, rtx, samples, name, n=200):
    """prims_sets.query_set's rays and point pairs, answered on this pose's oracle scene"""
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
    return qs._once("moves_query_" + name, make)


def hard_rays(orc, rtx, samples):
    """THE hard-ray set: 33 rays straight down onto the turned cluster, each with a -0.0 component, answered by the own tree
    of the oracle scene created with `turn`'s primitives, and the answers of their +0.0 twins"""
    def make():
        osc = posed(orc, rtx, samples, "turn")["osc"]
        c = cluster_centre(rtx)
        rng = np.random.default_rng(12)
        o = (c + np.concatenate([rng.uniform(-25.0, 25.0, (33, 1)), np.full((33, 1), 90.0), rng.uniform(-25.0, 25.0, (33, 1))],
                                axis=1)).astype(F)
        d = np.tile(np.array([-0.0, -1.0, 0.125], F), (33, 1))
        d[::3, 2] = -0.0
        d[::3, 0] = 0.0625
        exp, _ = qs.oracle_hits(orc, osc, o, d, qs.HIT_DTYPE)
        twin, _ = qs.oracle_hits(orc, osc, o, np.where(d == 0, F(0.0), d).astype(F), qs.HIT_DTYPE)
        return o, d, exp, twin
    return qs._once("moves_hard", make)


# the exact sphere-triangle tie of prims_sets, reached by a move: the sphere follows a translation of (-5, 0, 0)
TIE_MOVES = dict(moves=translation((-5.0, 0.0, 0.0)).reshape(1, 12), group=np.array([NONE, 0, NONE], np.uint32), radius_scale=None)


# ---- the count scenes: prims_sets.size_scenes' 255 / 256 / 257 primitives, every third a sphere
COUNTS = ("mixed255", "mixed256", "mixed257")


def count_moves(n_prims, many=False):
    """many: a move per primitive, translations of k x 0.01; else four moves dealt by Vec position, every fifth NONE"""
    k = np.arange(n_prims)
    if many:
        m = np.stack([translation((0.01 * i, -0.01 * i, 0.005 * i)) for i in k]).astype(F)
        return dict(moves=m, group=k.astype(np.uint32), radius_scale=None)
    a = np.deg2rad(10.0)        # (gentle maps: the count scenes' bound is 200)
    m = np.stack([translation((3.0, -2.0, 1.5)), about([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]], np.array([-15.0, 100.0, 0.0])),
                  about(np.diag([0.5, 0.9, -1.0]), np.array([-10.0, 90.0, 5.0])), IDENTITY]).astype(F)
    group = np.where(k % 5 == 4, NONE, k % 4).astype(np.uint32)
    return dict(moves=m, group=group, radius_scale=np.array([1.5, 0.25, 1.0, 3.0], F))


def count_cases(rtx):
    """(name, scene dict, moves keywords): the three count scenes under the dealt moves, and `many` on the 257"""
    sizes = pm.size_scenes(rtx)
    out = [(n, sizes[n], count_moves(len(sizes[n]["kinds"]))) for n in COUNTS]
    out.append(("many", sizes["mixed257"], count_moves(257, many=True)))
    return out
