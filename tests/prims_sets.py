"""Fixtures for the rtx_scene_pose_prims tests — a pose that states every field of every primitive — with the CPU oracle's
answers: numpy, the oracle binding and the library's host side only, no GPU.

The main fixture, "yard", is a 24 x 16 frame with two rays per pixel and ten light samples, main()'s kind of camera and
light: the ground triangle (global), 40 triangles of rtx.synthetic_mesh drawn together and enlarged into a cluster, and 5
spheres interleaved through `kinds`, so that Vec positions, triangle numbers and sphere numbers all differ.  A pose's
expected values come from an ORACLE SCENE CREATED WITH THE POSED PRIMITIVES, as pose_sets.posed does it.
tests/test_prims_sets.py asserts, without a GPU, the conditions the fixtures must meet; tests/test_prims_host.py and
tests/test_gpu_prims.py use them.  Everything is built once per process (query_sets._once)."""
import numpy as np

import query_sets as qs
import shade_sets as ss
import view_sets as vs
from query_sets import F

YARD_VIEW = ((24, 16), (0.0, 110.0, 210.0), (0.0, 20.0, 0.0), 26.0)
NB_RAY, NB_LIGHT = 2, 10
N_MESH, N_SPHERES = 40, 5
GROUND_NUMBER = 17                          # the ground's triangle number; its Vec position is another (GROUND_AT)
SPHERE_AT = (2, 9, 21, 30, 45)              # Vec positions of the spheres
N_PRIMS = N_MESH + 1 + N_SPHERES
POSES = ("move", "radius", "recolour", "all", "identity")
TURN_DEGREES = 40.0
RECOLOURED_TRIS = (1, 5, 8, 19, 24, 37)     # triangle numbers (the ground aside) that `recolour` paints
RECOLOURED_SPHERES = (1, 3)
SPHERES = np.array([[-70.0, 14.0, 30.0, 14.0], [60.0, 12.0, 40.0, 12.0], [-40.0, 10.0, 90.0, 10.0], [50.0, 16.0, -40.0, 16.0],
                    [30.0, 9.0, 70.0, 9.0]], F)
SPHERE_RGB = np.array([[0.9, 0.3, 0.2], [0.2, 0.8, 0.3], [0.3, 0.4, 0.9], [0.9, 0.8, 0.2], [0.7, 0.7, 0.7]], F)
POSE_LIGHT = ((-260.0, 280.0, 30.0, -240.0, 280.0, 30.0, -250.0, 280.0, 50.0), 7)      # the light of the lit posed view


def kinds():
    k = np.zeros(N_PRIMS, np.uint8)
    k[list(SPHERE_AT)] = 1
    return k


GROUND_AT = int(np.nonzero(kinds() == 0)[0][GROUND_NUMBER])


def yard(rtx):
    """the uploaded primitives: dict(tris [41, 9], rgb [41, 3], spheres [5, 4], sphere_rgb [5, 3], kinds [46])"""
    def make():
        soup = rtx.synthetic_mesh(N_MESH).astype(np.float64).reshape(-1, 3, 3)
        c = soup.mean(axis=1, keepdims=True)
        mesh = (c - np.array([-16.0, 105.0, -2.0])) * np.array([0.45, 0.4, 0.45]) + np.array([-5.0, 36.0, 0.0]) + (soup - c) * 14.0
        ground = np.asarray(rtx.GROUND_TRI, np.float64).reshape(1, 3, 3)
        tris = np.concatenate([mesh[:GROUND_NUMBER], ground, mesh[GROUND_NUMBER:]]).reshape(-1, 9).astype(F)
        rgb = np.linspace(0.25, 1.0, 3 * (N_MESH + 1), dtype=F).reshape(-1, 3)
        rgb[GROUND_NUMBER] = (0.5, 0.5, 0.5)
        out = dict(tris=np.ascontiguousarray(tris), rgb=np.ascontiguousarray(rgb), spheres=SPHERES.copy(),
                   sphere_rgb=SPHERE_RGB.copy(), kinds=kinds())
        for a in out.values():
            a.setflags(write=False)
        return out
    return qs._once("prims_yard", make)


def turned(tris, degrees):
    """every triangle but the ground turned about the vertical through the cluster's box centre"""
    out = np.array(tris, np.float64).reshape(-1, 3, 3)
    mesh = np.ones(len(out), bool)
    mesh[GROUND_NUMBER] = False
    pts = out[mesh].reshape(-1, 3)
    c = 0.5 * (pts.min(axis=0) + pts.max(axis=0))
    a = np.deg2rad(degrees)
    x, z = out[mesh, :, 0] - c[0], out[mesh, :, 2] - c[2]
    out[mesh, :, 0], out[mesh, :, 2] = c[0] + np.cos(a) * x + np.sin(a) * z, c[2] - np.sin(a) * x + np.cos(a) * z
    return np.ascontiguousarray(out.reshape(-1, 9).astype(F))


def moved_spheres():
    s = SPHERES.copy()
    s[0, [0, 2]], s[1, [0, 2]] = SPHERES[1, [0, 2]], SPHERES[0, [0, 2]]      # two change place with each other
    s[2, :3] = (2.0, 20.0, 40.0)                                             # one rolls in front of the cluster
    s[3, :3] = (88.0, 16.0, 20.0)                                            # one to where its shadow falls on other ground
    return s


def resized_spheres(s):
    s = s.copy()
    s[3, 1], s[3, 3] = 2.0 * s[3, 3], 2.0 * s[3, 3]                          # one doubles (and stays on the ground)
    s[4, 3] = 0.0                                                            # one shrinks to radius 0
    return s


def recoloured(rgb, sphere_rgb):
    rgb, sphere_rgb = rgb.copy(), sphere_rgb.copy()
    rgb[GROUND_NUMBER] = (0.8, 0.45, 0.3)
    for k, n in enumerate(RECOLOURED_TRIS):
        rgb[n + (n >= GROUND_NUMBER)] = (0.15 + 0.1 * k, 0.9 - 0.12 * k, 0.2 + 0.05 * k)
    sphere_rgb[list(RECOLOURED_SPHERES)] = ((0.1, 0.2, 0.95), (0.95, 0.15, 0.6))
    return rgb, sphere_rgb


def yard_pose(rtx, name):
    """the posed primitives, every array in full: dict(tris, rgb, spheres, sphere_rgb)"""
    y = yard(rtx)
    p = dict(tris=y["tris"].copy(), rgb=y["rgb"].copy(), spheres=y["spheres"].copy(), sphere_rgb=y["sphere_rgb"].copy())
    if name == "move":
        p["spheres"] = moved_spheres()
    elif name == "radius":
        p["spheres"] = resized_spheres(y["spheres"])
    elif name == "recolour":
        p["rgb"], p["sphere_rgb"] = recoloured(y["rgb"], y["sphere_rgb"])
    elif name == "all":
        p["spheres"] = resized_spheres(moved_spheres())
        p["rgb"], p["sphere_rgb"] = recoloured(y["rgb"], y["sphere_rgb"])
        p["tris"] = turned(y["tris"], TURN_DEGREES)
    elif name != "identity":
        raise KeyError(name)
    return {k: np.ascontiguousarray(v, F) for k, v in p.items()}


def given(rtx, name):
    """keywords of rtx.Scene.pose_prims for the pose: the arrays the pose changes (identity and all: every array), the
    others None — as uploaded"""
    p = yard_pose(rtx, name)
    keep = dict(move=("spheres",), radius=("spheres",), recolour=("rgb", "sphere_rgb"))
    kw = dict(v0v1v2=p["tris"], spheres=p["spheres"], rgb=p["rgb"], sphere_rgb=p["sphere_rgb"])
    if name in keep:
        kw.update({k: None for k in ("spheres", "rgb", "sphere_rgb") if k not in keep[name]})
    return kw


def left_as_uploaded(rtx, name, part):
    """the posed primitives with one part — "spheres" or "colours" — left as uploaded"""
    y, p = yard(rtx), dict(yard_pose(rtx, name))
    if part == "spheres":
        p["spheres"] = y["spheres"].copy()
    else:
        p["rgb"], p["sphere_rgb"] = y["rgb"].copy(), y["sphere_rgb"].copy()
    return p


def oracle_scene(orc, samples, prims, view=YARD_VIEW, **kw):
    more = dict(dict(nb_ray=NB_RAY, nb_light_sample=NB_LIGHT, spheres=prims["spheres"], sphere_rgb=prims["sphere_rgb"], kinds=kinds()),
                **kw)
    return orc.Scene(view[0][0], view[0][1], prims["tris"], prims["rgb"], samples[:4096], **dict(vs.camera(view), **more))


def render(orc, samples, prims, **kw):
    """-> dict(osc, frame, stats, tri = one ray's hit primitive per pixel, lin)"""
    osc = oracle_scene(orc, samples, prims, **kw)
    frame, st, tri, lin = osc.render_rows(mode=orc.MODE_BVH, want_tri=True, want_lin=True)
    for a in (frame, tri, lin):
        a.setflags(write=False)
    return dict(osc=osc, frame=frame, stats=st, tri=tri, lin=lin)


def posed(orc, rtx, samples, name):
    def make():
        prims = yard_pose(rtx, name)
        return dict(render(orc, samples, prims), prims=prims)
    return qs._once("prims_posed_" + name, make)


def without(orc, rtx, samples, name, part):
    return qs._once("prims_without_%s_%s" % (name, part), lambda: render(orc, samples, left_as_uploaded(rtx, name, part)))


def lit_frame(orc, rtx, samples, name):
    def make():
        tri, count = POSE_LIGHT
        r = render(orc, samples, yard_pose(rtx, name), light_tri=tri, nb_light_sample=count)
        r["osc"].close()
        return r["frame"], r["stats"]
    return qs._once("prims_lit_" + name, make)


def open_yard(rtx, samples, **kw):
    """the library's scene of the uploaded yard, created with the default camera's kind of frame (8 x 8: every call here
    brings its own view)"""
    y = yard(rtx)
    more = dict(dict(nb_ray=NB_RAY, nb_light_sample=NB_LIGHT, reference_tree=rtx.REFTREE_NEVER, tie_rank=None), **kw)
    return rtx.Scene(8, 8, y["tris"], y["rgb"], samples[:4096], spheres=y["spheres"], sphere_rgb=y["sphere_rgb"], kinds=y["kinds"],
                     **dict(vs.camera(YARD_VIEW), **more))


def tables(orc, rtx, name):
    def make():
        p = yard_pose(rtx, name)
        return ss.prim_tables(orc, p["tris"], p["rgb"], p["spheres"], p["sphere_rgb"], kinds())
    return qs._once("prims_tables_" + name, make)


def composition(orc, rtx, samples, name):
    """render_pixel composed from oracle pieces on the posed oracle scene for the yard view's rays (shade and hit records)"""
    def make():
        (w, h), eye, look_at, distance = YARD_VIEW
        o, d, _, _, _ = ss.camera_raw_rays(orc, w, h, eye, look_at, vs.UP, distance, samples[:4096], NB_RAY)
        return ss.shade_set(orc, posed(orc, rtx, samples, name)["osc"], o, d, NB_RAY, NB_LIGHT, orc.LIGHT_TRI, samples[:4096],
                            tables(orc, rtx, name))
    return qs._once("prims_comp_" + name, make)


def query_set(orc, rtx, samples, name, n=200):
    """200 random rays into the yard and 200 point pairs from the same origins, answered on the posed oracle scene:
    (origins, directions, expected hits), (origins, targets, expected hits of the pairs' rays, expected occlusion bytes)"""
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
    return qs._once("prims_query_" + name, make)


def hard_rays(orc, rtx, samples):
    """33 rays straight down onto the sphere `move` rolls in front of the cluster, each with a -0.0 component, answered by
    the posed oracle scene's own tree, and the answers of their +0.0 twins"""
    def make():
        osc = posed(orc, rtx, samples, "move")["osc"]
        c = moved_spheres()[2]
        rng = np.random.default_rng(12)
        o = (c[:3] + np.concatenate([rng.uniform(-0.9, 0.9, (33, 1)) * c[3], np.full((33, 1), 90.0), rng.uniform(-0.9, 0.9, (33, 1)) * c[3]],
                                    axis=1)).astype(F)
        d = np.tile(np.array([-0.0, -1.0, 0.125], F), (33, 1))
        d[::3, 2] = -0.0
        d[::3, 0] = 0.0625
        exp, _ = qs.oracle_hits(orc, osc, o, d, qs.HIT_DTYPE)
        twin, _ = qs.oracle_hits(orc, osc, o, np.where(d == 0, F(0.0), d).astype(F), qs.HIT_DTYPE)
        return o, d, exp, twin
    return qs._once("prims_hard", make)


# ---- the tie: a sphere the pose moves so that a ray meets it and a triangle at exactly the same distance
TIE_TRIS = np.array([[-1, -1, -6, 1, -1, -6, 0, 1, -6], [3, 3, -9, 4, 3, -9, 3, 4, -9]], F)
TIE_SPHERES = np.array([[5, 0, -8, 2]], F)
TIE_MOVED = np.array([[0, 0, -8, 2]], F)
TIE_KINDS = np.array([0, 1, 0], np.uint8)                   # Vec positions: triangle 0, the sphere, triangle 1
TIE_RAY = (np.array([[0.0, 0.0, 0.0]], F), np.array([[0.0, 0.0, -1.0]], F))
TIE_KW = dict(eye=(0.0, 0.0, 0.0), look_at=(0.0, 0.0, -1.0), up=(0.0, 1.0, 0.0), distance=8.0,
              light_tri=(-2.0, 9.0, -3.0, 2.0, 9.0, -3.0, 0.0, 9.0, 1.0), nb_light_sample=4)


# ---- scenes for the record comparisons at the sizes at which indexing can go wrong:
#      name -> dict(tris, rgb, spheres, sphere_rgb, kinds, kw, pose = dict(tris, rgb, spheres, sphere_rgb))
def _redrawn(rtx, tris, spheres, seed):
    rng = np.random.default_rng(seed)
    pose = dict(tris=np.ascontiguousarray(rtx.synthetic_mesh(len(tris), seed=777)) if len(tris) else np.zeros((0, 9), F),
                rgb=rng.uniform(0.0, 1.0, (len(tris), 3)).astype(F),
                spheres=np.concatenate([rng.uniform(-60, 60, (len(spheres), 3)), rng.uniform(0.0, 5.0, (len(spheres), 1))], axis=1).astype(F),
                sphere_rgb=rng.uniform(0.0, 1.0, (len(spheres), 3)).astype(F))
    return pose


def size_scenes(rtx, leaf_max=4):
    def make():
        out = {}
        rng = np.random.default_rng(41)

        def scene(n_tris, n_spheres, kinds, **kw):
            tris = rtx.synthetic_mesh(n_tris) if n_tris else np.zeros((0, 9), F)
            spheres = np.concatenate([rng.uniform(-80, 50, (n_spheres, 1)), rng.uniform(35, 170, (n_spheres, 1)),
                                      rng.uniform(-55, 55, (n_spheres, 1)), rng.uniform(0.5, 4.0, (n_spheres, 1))], axis=1).astype(F)
            return dict(tris=tris, rgb=np.linspace(0.1, 1.0, 3 * n_tris, dtype=F).reshape(-1, 3), spheres=spheres,
                        sphere_rgb=np.linspace(1.0, 0.2, 3 * n_spheres, dtype=F).reshape(-1, 3), kinds=kinds, kw=kw,
                        pose=_redrawn(rtx, tris, spheres, 100 + n_tris + n_spheres))
        for n in (255, 256, 257):                           # every third primitive a sphere
            k = (np.arange(n) % 3 == 2).astype(np.uint8)
            out["mixed%d" % n] = scene(int((k == 0).sum()), int(k.sum()), k)
        out["mixed257_brute"] = dict(out["mixed257"], kw=dict(accel=rtx.ACCEL_BRUTE))
        out["spheres_only"] = scene(0, 13, np.ones(13, np.uint8))
        for n in (1, leaf_max, leaf_max + 1):               # the sphere run of the rebuilt shape
            k = np.concatenate([np.zeros(9, np.uint8), np.ones(n, np.uint8)])
            out["nine_and_%d" % n] = scene(9, n, k)
        return out
    return qs._once("prims_sizes_%d" % leaf_max, make)


def open_sized(rtx, samples, sc, **more):
    return rtx.Scene(8, 8, sc["tris"], sc["rgb"], samples[:4096], spheres=sc["spheres"] if len(sc["spheres"]) else None,
                     sphere_rgb=sc["sphere_rgb"] if len(sc["spheres"]) else None, kinds=sc["kinds"], nb_light_sample=4,
                     **dict(dict(reference_tree=rtx.REFTREE_NEVER, tie_rank=None), **dict(sc["kw"], **more)))


def pose_kw(pose):
    """a pose dict as keywords of rtx.Scene.pose_prims*"""
    return dict(v0v1v2=pose["tris"], spheres=pose["spheres"], rgb=pose["rgb"], sphere_rgb=pose["sphere_rgb"])
