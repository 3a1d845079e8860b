"""Poses for the rtx_scene_pose tests, with the CPU oracle's answers: numpy, the oracle binding and the library's host
side only, no GPU.

A pose is float32 [n_tris, 9] in the layout of RtxSceneDesc.v0v1v2.  The bunny poses are on big_bunny + ground (the
ground is Vec position 4968, the pose bound M = 10000) seen through view_sets' "side" view, 44 x 27; their expected
values come from an ORACLE SCENE CREATED WITH THE POSED VERTICES, everything else the uploaded scene's.  The small scenes
are for the record comparisons (rtx_scene_posed_records against rtx_debug_pose and against numpy).
tests/test_pose_sets.py asserts, without a GPU, the conditions the fixtures must meet; tests/test_pose_host.py and
tests/test_gpu_pose.py use them.  Everything is built once per process (query_sets._once)."""
import numpy as np

import light_sets as ls
import query_sets as qs
import shade_sets as ss
import view_sets as vs
from query_sets import F, NO_HIT

M = 10000.0
GROUND = 4968
SIDE = vs.BUNNY_VIEWS["side"]
BUNNY_POSES = ("identity", "turn", "shift", "squash", "tilt")
SHIFT = (120.0, 0.0, -80.0)
TURNTABLE_DEGREES = (25.0, 115.0, 205.0, 295.0)
TURNTABLE_VIEW = ((24, 16), (320.0, 140.0, 40.0), (-20.0, 70.0, 0.0), 16.0)
POSE_LIGHT = "far_side"                    # light_sets.SIDE_LIGHTS' name of the light the lit posed view is rendered under
LEAF_MASK, LEAF_FLAG = 0x3FFFFFFF, 0x80000000


def base(orc):
    """(tris [4969, 9], rgb [4969, 3]) of big_bunny + ground"""
    return qs._once("pose_base", lambda: orc.default_primitives(["big_bunny.obj"]))


def turned(tris, degrees):
    """the mesh (every row but the ground's) turned about the vertical through its box centre"""
    out = np.array(tris, np.float64).reshape(-1, 3, 3)
    mesh = out[:GROUND]
    c = 0.5 * (mesh.reshape(-1, 3).min(axis=0) + mesh.reshape(-1, 3).max(axis=0))
    a = np.deg2rad(degrees)
    x, z = mesh[..., 0] - c[0], mesh[..., 2] - c[2]
    mesh[..., 0], mesh[..., 2] = c[0] + np.cos(a) * x + np.sin(a) * z, c[2] - np.sin(a) * x + np.cos(a) * z
    return np.ascontiguousarray(out.reshape(-1, 9).astype(F))


def bunny_pose(orc, name):
    tris = base(orc)[0]
    if name == "identity":
        return np.ascontiguousarray(tris.copy())
    if name == "turn":
        return turned(tris, 40.0)
    out = np.array(tris, np.float64).reshape(-1, 3, 3)
    if name == "shift":
        out[:GROUND] += np.asarray(SHIFT)
    elif name == "squash":
        y = out[:GROUND, :, 1].copy()
        out[:GROUND, :, 1] = 0.5 * y
        out[:GROUND, :, 0] += 12.0 * np.sin(y / 25.0)
    elif name == "tilt":
        out = np.array(turned(tris, 15.0), np.float64).reshape(-1, 3, 3)
        out[GROUND, :, 1] += 0.002 * out[GROUND, :, 0]
    else:
        raise KeyError(name)
    return np.ascontiguousarray(out.reshape(-1, 9).astype(F))


def oracle_scene(orc, samples, tris, v, **kw):
    return orc.Scene(v[0][0], v[0][1], tris, base(orc)[1], samples, **dict(vs.camera(v), **kw))


def posed(orc, samples, name):
    """-> dict(pose, osc = the oracle scene created with the posed vertices and the side view, frame, stats, tri = the
    hit primitive per pixel, normals = orc_triangle_new's per triangle)"""
    def make():
        pose = bunny_pose(orc, name)
        osc = oracle_scene(orc, samples, pose, SIDE)
        frame, st, tri, lin = osc.render_rows(mode=orc.MODE_BVH, want_tri=True, want_lin=True)
        for a in (pose, frame, tri, lin):
            a.setflags(write=False)
        return dict(pose=pose, osc=osc, frame=frame, stats=st, tri=tri, lin=lin)
    return qs._once("pose_" + name, make)


def tables(orc, samples, name):
    def make():
        return ss.prim_tables(orc, posed(orc, samples, name)["pose"], base(orc)[1])
    return qs._once("pose_tables_" + name, make)


def composition(orc, samples, name, light=None):
    """render_pixel composed from oracle pieces on the posed oracle scene for the side view's rays (shade and hit records),
    under the scene's light or light_sets.SIDE_LIGHTS[light]"""
    def make():
        p = posed(orc, samples, name)
        (w, h), eye, look_at, distance = SIDE
        o, d, _, _, _ = ss.camera_raw_rays(orc, w, h, eye, look_at, vs.UP, distance, samples, 1)
        tri, count = (orc.LIGHT_TRI, orc.NB_LIGHT_SAMPLE) if light is None else ls.SIDE_LIGHTS[light]
        s = ss.shade_set(orc, p["osc"], o, d, 1, count, tri, samples, tables(orc, samples, name))
        s.update(light=tuple(tri), count=count)
        return s
    return qs._once("pose_comp_%s_%s" % (name, light), make)


def lit_frame(orc, samples, name, light):
    """(frame, stats) of an oracle scene created with the posed vertices, the side view and light_sets.SIDE_LIGHTS[light]"""
    def make():
        tri, count = ls.SIDE_LIGHTS[light]
        osc = oracle_scene(orc, samples, posed(orc, samples, name)["pose"], SIDE, light_tri=tri, nb_light_sample=count)
        frame, st = osc.render_rows(mode=orc.MODE_BVH)
        osc.close()
        return frame, st
    return qs._once("pose_lit_%s_%s" % (name, light), make)


def query_set(orc, samples, name, n=300):
    """query_sets' random bunny rays and point pairs (the first n) answered on the posed oracle scene:
    (origins, directions, expected hits), (origins, targets, expected hits of the pairs' rays, expected occlusion bytes)"""
    def make():
        osc = posed(orc, samples, name)["osc"]
        sets = qs.bunny(orc, samples)["sets"]
        ro, rd = sets["random"][0][:n], sets["random"][1][:n]
        exp, _ = qs.oracle_hits(orc, osc, ro, rd, qs.HIT_DTYPE)
        to, tt = sets["random_targets"][0][:n], sets["random_targets"][1][:n]
        texp, _ = qs.oracle_hits(orc, osc, to, (tt - to).astype(F), qs.HIT_DTYPE)
        return (ro, rd, exp), (to, tt, texp, qs.expected_occlusion(texp, to, tt))
    return qs._once("pose_query_" + name, make)


def hard_rays(orc, samples, name):
    """64 + 7 rays straight down onto the posed mesh with a -0.0 x component (the named hard-ray set), answered by the
    oracle scene's own tree, and the answers of their +0.0 twins"""
    def make():
        p = posed(orc, samples, name)
        mesh = p["pose"][:GROUND].reshape(-1, 3)
        lo, hi = mesh.min(axis=0), mesh.max(axis=0)
        rng = np.random.default_rng(11)
        o = rng.uniform((lo[0], hi[1] + 20.0, lo[2]), (hi[0], hi[1] + 30.0, hi[2]), size=(71, 3)).astype(F)
        d = np.tile(np.array([-0.0, -1.0, 0.25], F), (71, 1))
        d[::3, 2] = -0.0
        d[::3, 0] = 0.125
        exp, _ = qs.oracle_hits(orc, p["osc"], o, d, qs.HIT_DTYPE)
        twin, _ = qs.oracle_hits(orc, p["osc"], o, np.where(d == 0, F(0.0), d).astype(F), qs.HIT_DTYPE)
        return o, d, exp, twin
    return qs._once("pose_hard_" + name, make)


def turntable(orc, samples):
    """[(pose, oracle frame)] for the mesh at TURNTABLE_DEGREES, 24 x 16"""
    def make():
        out = []
        for deg in TURNTABLE_DEGREES:
            pose = turned(base(orc)[0], deg)
            osc = oracle_scene(orc, samples, pose, TURNTABLE_VIEW)
            frame, _ = osc.render_rows(mode=orc.MODE_BVH)
            osc.close()
            out.append((pose, frame))
        return out
    return qs._once("pose_turntable", make)


# ---- the tie: two triangles the pose makes coincide, and a third elsewhere
TIE_TRIS = np.array([[-1, -1, -5, 1, -1, -5, 0, 1, -5], [-1, -1, -7, 1, -1, -7, 0, 1, -7], [3, 3, -9, 4, 3, -9, 3, 4, -9]], F)
TIE_POSE = np.array([[-1, -1, -6, 1, -1, -6, 0, 1, -6], [-1, -1, -6, 1, -1, -6, 0, 1, -6], [3, 3, -9, 4, 3, -9, 3, 4, -8]], F)
TIE_RAYS = (np.array([[0.0, 0.0, 0.0], [0.1, -0.2, 1.0]], F), np.array([[0.01, -0.02, -1.0], [0.02, 0.03, -1.0]], F))
TIE_KW = dict(eye=(0.0, 0.0, 0.0), look_at=(0.0, 0.0, -1.0), up=(0.0, 1.0, 0.0), distance=8.0,
              light_tri=(-2.0, 9.0, -3.0, 2.0, 9.0, -3.0, 0.0, 9.0, 1.0), nb_light_sample=4)


# ---- small scenes for the record comparisons: name -> (tris, spheres or None, kinds or None, keywords, pose)
def small_scenes(rtx):
    def make():
        out = {}
        one = np.array([[0, 0, -5, 1, 0, -5, 0, 1, -5]], F)
        out["one"] = (one, None, None, {}, np.array([[0.5, 0, -6, 2, 0.25, -6, 0, 3, -7]], F))
        two = np.array([[-3, 0, -8, -1, 0, -8, -2, 2, -8], [1, 0, -9, 3, 0, -9, 2, 2, -9]], F)
        out["sphere_between"] = (two, np.array([[0, 1, -8, 1]], F), np.array([0, 1, 0], np.uint8), {},
                                 np.ascontiguousarray(two[::-1] + F(0.5)))
        for n in (255, 256, 257):
            soup, redrawn = rtx.synthetic_mesh(n), rtx.synthetic_mesh(n, seed=777)
            out["soup%d" % n] = (soup, None, None, {}, redrawn)
            out["soup%d_brute" % n] = (soup, None, None, dict(accel=rtx.ACCEL_BRUTE), redrawn)
            g = np.concatenate([soup, np.asarray(rtx.GROUND_TRI, F).reshape(1, 9)])
            gp = np.concatenate([redrawn, np.asarray(rtx.GROUND_TRI, F).reshape(1, 9) * F(0.5)])
            out["soup%d_ground" % n] = (g, None, None, {}, np.ascontiguousarray(gp))
        return out
    return qs._once("pose_small", make)


def open_small(rtx, samples, scene, **more):
    tris, spheres, kinds, kw, _ = scene
    rgb = np.linspace(0.1, 1.0, 3 * len(tris), dtype=F).reshape(-1, 3)
    return rtx.Scene(8, 8, tris, rgb, samples[:4096], spheres=spheres, kinds=kinds, nb_light_sample=4,
                     **dict(dict(reference_tree=rtx.REFTREE_NEVER, tie_rank=None), **dict(kw, **more)))


def node_ranges(nodes):
    """(first, count) per node of rtx.Scene.nodes()' records, from the stream alone: a leaf names its run; an inner
    node's run spans the leaves of its subtree, records (i, link_i)"""
    info, link = nodes[:, 7].astype(np.int64), nodes[:, 3].astype(np.int64)
    leaf = (info & LEAF_FLAG) != 0
    first = np.where(leaf, info & LEAF_MASK, np.iinfo(np.int64).max)
    end = np.where(leaf, (info & LEAF_MASK) + link, -1)
    out = np.zeros((len(nodes), 2), np.int64)
    for i in range(len(nodes)):
        if leaf[i]:
            out[i] = first[i], link[i]
        else:
            lo, hi = first[i + 1:link[i]].min(), end[i + 1:link[i]].max()
            out[i] = lo, hi - lo
    return out


def numpy_fold(tris_words, nodes, cull_delta):
    """[n_nodes, 6] float32: min / max of the posed own boxes (words 9-11, 12-14 of a primitive record) over every node's
    run, moved outwards by cull_delta in float32"""
    t = tris_words.view(F)
    lo, hi = t[:, 9:12], t[:, 12:15]
    out = np.zeros((len(nodes), 6), F)
    for i, (first, count) in enumerate(node_ranges(nodes)):
        out[i, :3] = lo[first:first + count].min(axis=0) - F(cull_delta)
        out[i, 3:] = hi[first:first + count].max(axis=0) + F(cull_delta)
    return out


def cull_delta(bound):
    """PreparedScene::cull_delta from the pose bound, float32"""
    return F(F(bound) * F(2.0 ** -19) + F(2.0 ** -100))
