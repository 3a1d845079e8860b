"""Fixtures for the tests of rtx_scene_pose_rebuilt (a pose whose tree is rebuilt on the device): numpy, the oracle binding
and the library's host side only, no GPU.  pose_sets (the five bunny poses at the 44 x 27 "side" view, its small scenes, the
tie, the hard rays, the turntable) and posed_rows_sets (the lifted ground) serve as they are; what is added here:

SHAPE SCENES, the sizes at which the closed-form shape can go wrong, each with and without a ground: a tree proper of 0
records (the ground alone), 1, 2, leaf_max, leaf_max + 1, 2 leaf_max + 1, 255 / 256 / 257 (pose_sets' soups), one run of
exactly POSE_LANE_MAX records and one of POSE_LANE_MAX + 1, two triangles around a sphere, spheres only, coincident
triangles (equal keys), and the 20,000-triangle soup.

SCATTER, the pose DESIGN section 17 names: the 20,000-triangle soup re-drawn with another seed, with the ground, seen
36 x 33.

Also here: numpy restatements of the key (scene_prep.h: rebuild_key_statement), of the shape (rebuild_tables) and of the
surface-area cost of a stream.  tests/test_rebuild_sets.py asserts, without a GPU, the conditions the fixtures must meet;
tests/test_rebuild_host.py and tests/test_gpu_rebuild.py use them.  Everything is built once per process."""
import numpy as np

import pose_sets as ps
import query_sets as qs
import view_sets as vs
from query_sets import F

LEAF_MAX = 4                               # the library's default (RtxSceneDesc.leaf_max == 0)
CELL_BITS, CELL_MAX = 21, (1 << 21) - 1
SCATTER_N, SCATTER_SEED = 20000, 4242
SCATTER_VIEW = ((36, 33), (260.0, 210.0, 330.0), (-15.0, 75.0, 0.0), 200.0)
SCATTER_LIGHT = dict(nb_light_sample=6)


GROUND_TRI = (-10000.0, 0.0, -10000.0, 10000.0, 0.0, -10000.0, 0.0, 0.0, 10000.0)


def ground():
    return np.asarray(GROUND_TRI, F).reshape(1, 9)


# ---- the shape scenes: name -> (tris, spheres or None, kinds or None, keywords, pose), pose_sets.small_scenes' layout
def shape_scenes(rtx):
    def make():
        out = {}
        small = ps.small_scenes(rtx)
        for name in ("one", "sphere_between", "soup255", "soup256", "soup257", "soup255_ground", "soup256_ground",
                     "soup257_ground", "soup255_brute"):
            out[name] = small[name]
        g = ground()

        def with_ground(tris, pose):
            return np.ascontiguousarray(np.concatenate([tris, g])), np.ascontiguousarray(np.concatenate([pose, g * F(0.5)]))

        out["ground_alone"] = (g.copy(), None, None, {}, np.ascontiguousarray(g * F(0.5)))
        one, one_pose = small["one"][0], small["one"][4]
        t, p = with_ground(one, one_pose)
        out["one_ground"] = (t, None, None, {}, p)
        for n in (2, LEAF_MAX, LEAF_MAX + 1, 2 * LEAF_MAX + 1, rtx.rtx.POSE_LANE_MAX, rtx.rtx.POSE_LANE_MAX + 1):
            soup, redrawn = rtx.synthetic_mesh(n, seed=100 + n), rtx.synthetic_mesh(n, seed=900 + n)
            out["soup%d" % n] = (soup, None, None, {}, redrawn)
            t, p = with_ground(soup, redrawn)
            out["soup%d_ground" % n] = (t, None, None, {}, p)
        two, sph, kinds, kw, pose = small["sphere_between"]
        t, p = with_ground(two, pose)
        out["sphere_between_ground"] = (t, sph, np.array([0, 1, 0, 0], np.uint8), {}, p)
        # spheres beside one small triangle that the pose moves: eleven spheres, so that the sphere run splits
        rng = np.random.default_rng(21)
        spheres = np.concatenate([rng.uniform(-40, 40, (11, 3)), rng.uniform(0.5, 3.0, (11, 1))], axis=1).astype(F)
        out["spheres"] = (small["one"][0], spheres, np.array([1] * 5 + [0] + [1] * 6, np.uint8), {}, small["one"][4])
        # coincident triangles: six copies of one triangle among others, and a pose that makes eight coincide elsewhere
        soup = rtx.synthetic_mesh(20, seed=55)
        soup[3:9] = soup[3]
        pose = rtx.synthetic_mesh(20, seed=56)
        pose[2:10] = pose[12]
        out["coincident"] = (np.ascontiguousarray(soup), None, None, {}, np.ascontiguousarray(pose))
        t, p = with_ground(soup, pose)
        out["coincident_ground"] = (t, None, None, {}, p)
        return out
    return qs._once("rebuild_shapes", make)


def scatter(rtx):
    """(tris, pose) of the scatter scene WITH the ground: the 20,000-triangle soup and the soup re-drawn with another seed"""
    def make():
        g = ground()
        soup, redrawn = rtx.synthetic_mesh(SCATTER_N), rtx.synthetic_mesh(SCATTER_N, seed=SCATTER_SEED)
        out = np.ascontiguousarray(np.concatenate([soup, g])), np.ascontiguousarray(np.concatenate([redrawn, g]))
        for a in out:
            a.setflags(write=False)
        return out
    return qs._once("rebuild_scatter", make)


def scatter_rgb():
    rgb = np.tile(np.array([1.0, 1.0, 1.0], F), (SCATTER_N + 1, 1))
    rgb[-1] = (0.5, 0.5, 0.5)
    return np.ascontiguousarray(rgb)


def scatter_scene(rtx, samples, **more):
    """the library's scene, created with the UNPOSED soup and SCATTER_VIEW's frame and camera"""
    kw = dict(dict(vs.camera(SCATTER_VIEW), reference_tree=rtx.REFTREE_NEVER, tie_rank=None, **SCATTER_LIGHT), **more)
    return rtx.Scene(SCATTER_VIEW[0][0], SCATTER_VIEW[0][1], scatter(rtx)[0], scatter_rgb(), samples, **kw)


def scattered(rtx, orc, samples):
    """dict(frame, stats) of the oracle scene created with the SCATTERED vertices, and still = the unposed oracle frame"""
    def make():
        (w, h) = SCATTER_VIEW[0]
        kw = dict(vs.camera(SCATTER_VIEW), **SCATTER_LIGHT)
        out = {}
        for key, tris in zip(("still", "frame"), scatter(rtx)):
            osc = orc.Scene(w, h, tris, scatter_rgb(), samples, **kw)
            frame, st = osc.render_rows(mode=orc.MODE_BVH)
            osc.close()
            frame.setflags(write=False)
            out[key] = frame
            out[key + "_stats"] = st
        return out
    return qs._once("rebuild_scattered", make)


# ---- restatements ----------------------------------------------------------------------------------------------------------
def key_scale(bound):
    """S = 2^21 / (2 M), rounded to float32 once"""
    return F(2097152.0 / (2.0 * float(bound)))


def numpy_keys(tris_words, spheres, bound):
    """rebuild_key_statement over primitive records (uint32 [n, 16]); spheres: bool [n] -> uint64 [n]"""
    t = np.asarray(tris_words).view(F)
    m, s = F(bound), key_scale(bound)
    keys = np.where(spheres, np.uint64(1) << np.uint64(63), np.uint64(0)).astype(np.uint64)
    with np.errstate(all="ignore"):
        for k in range(3):
            c = (F(0.5) * (t[:, 9 + k] + t[:, 12 + k]).astype(F)).astype(F)
            f = ((c + m).astype(F) * s).astype(F)
            q = np.where(f >= F(2097151.0), CELL_MAX, np.where(f >= 0, np.trunc(np.where(f >= 0, np.minimum(f, F(2097151.0)), 0)), 0))
            q = q.astype(np.uint64)
            for b in range(CELL_BITS):
                keys |= ((q >> np.uint64(b)) & np.uint64(1)) << np.uint64(3 * b + (2 - k))
    return keys


def shape(n_global, n_tris, n_spheres, leaf_max):
    """the rebuilt stream's (link, info) words and (first, count) runs, restated: lists of equal length"""
    LEAF, SPHERE = 0x80000000, 0x40000000
    link, info, runs = [], [], []

    def sub(begin, count, sphere):
        i = len(link)
        link.append(0), info.append(0), runs.append((begin, count))
        if count <= leaf_max:
            info[i], link[i] = LEAF | (SPHERE if sphere else 0) | begin, count
            return
        sub(begin, count // 2, sphere)
        info[i] = len(link)
        sub(begin + count // 2, count - count // 2, sphere)
        link[i] = len(link)

    def proper():
        if n_tris and n_spheres:
            i = len(link)
            link.append(0), info.append(0), runs.append((n_global, n_tris + n_spheres))
            sub(n_global, n_tris, False)
            info[i] = len(link)
            sub(n_global + n_tris, n_spheres, True)
            link[i] = len(link)
        elif n_tris:
            sub(n_global, n_tris, False)
        elif n_spheres:
            sub(n_global, n_spheres, True)

    if n_global:
        if n_tris + n_spheres:
            link.append(0), info.append(2), runs.append((0, n_global + n_tris + n_spheres))
            link.append(n_global), info.append(LEAF), runs.append((0, n_global))
            proper()
            link[0] = len(link)
        else:
            link.append(n_global), info.append(LEAF), runs.append((0, n_global))
    else:
        proper()
    return np.array(link, np.uint32), np.array(info, np.uint32), np.array(runs, np.int64).reshape(-1, 2)


def sah_cost(nodes, n_global):
    """Surface-area cost of a stream (uint32 [n, 8], NodeRec word order): sum over the nodes below the root of
    half_area(node) / half_area(root) x (1 for an inner node — one box test —, its record count for a leaf), as
    TreeBuilder::choose_split weighs a split (box cost 1, one unit per primitive).  The root is the stream's first record
    whose run is everything: with global triangles the root and the global leaf are left out (no ray tests them)."""
    f = nodes.view(F)
    info, link = nodes[:, 7], nodes[:, 3]
    leaf = (info & 0x80000000) != 0
    ext = np.maximum(f[:, 4:7].astype(np.float64) - f[:, 0:3].astype(np.float64), 0.0)
    half = ext[:, 0] * ext[:, 1] + ext[:, 1] * ext[:, 2] + ext[:, 2] * ext[:, 0]
    first = 2 if (n_global and len(nodes) > 2) else 0
    root = half[first]
    weight = np.where(leaf, link.astype(np.float64), 1.0)
    return float((half[first:] * weight[first:]).sum() / root)
