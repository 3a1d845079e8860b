"""Scenes and eyes for the tests of the aimed stream (rtx_scene_aimed_nodes on the host, rtx_debug_aimed_nodes on the
device), and an independent restatement of it: plain numpy, no GPU, no oracle.

The aimed stream is rtx_scene_nodes' stream with every plane moved outwards by cull_delta (f32) and, below the tree
proper's root, of every inner node's two children the one whose box centre is nearer the eye first."""
import os

import numpy as np

import view_sets as vs
from test_host_spheres import mixed_scene

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LEAF = 0x80000000
SCENES = ("bunny_ground", "soup", "one_triangle", "bunny_leaf1", "mirrored")
CREATED_EYE = {"bunny_ground": (0.0, 100.0, 200.0), "soup": (1.0, 2.0, 9.0), "one_triangle": (0.5, 0.25, 7.0),
               "bunny_leaf1": (0.0, 100.0, 200.0), "mirrored": (0.0, 3.0, 10.0)}
# two triangles that are each other's mirror image in the plane x = 0: from an eye on that plane their boxes' centres are
# exactly equally far
MIRRORED = np.array([[1.0, 0.0, 0.0, 2.0, 0.0, 0.5, 1.5, 1.0, 1.0],
                     [-1.0, 0.0, 0.0, -2.0, 0.0, 0.5, -1.5, 1.0, 1.0]], F)


def make_scene(rtx, name, samples):
    """-> (scene, coordinates whose largest magnitude, with the created eye's, is behind cull_delta)"""
    kw = dict(eye=CREATED_EYE[name], look_at=(0.0, 0.0, -20.0), distance=20.0, tie_rank=None, nb_light_sample=4)
    if name in ("bunny_ground", "bunny_leaf1"):
        tris, rgb = rtx.default_primitives([os.path.join(ROOT, "models", "bunny.obj")])
        scene = rtx.Scene(16, 12, tris, rgb, samples, leaf_max=1 if name == "bunny_leaf1" else 0, **kw)
        return scene, tris
    if name == "soup":
        tris, rgb, spheres, srgb, kinds = mixed_scene(np.random.default_rng(5), 120, 30)
        scene = rtx.Scene(16, 12, tris, rgb, samples, spheres=spheres, sphere_rgb=srgb, kinds=kinds, **kw)
        r = spheres[:, 3:4]
        return scene, np.concatenate([tris.reshape(-1), (spheres[:, :3] - r).astype(F).reshape(-1),
                                      (spheres[:, :3] + r).astype(F).reshape(-1)])
    if name == "one_triangle":
        tris = np.array([[0.0, 0.0, -3.0, 2.0, 0.5, -4.0, 1.0, 3.0, -2.5]], F)
        return rtx.Scene(16, 12, tris, np.ones((1, 3), F), samples, **kw), tris
    if name == "mirrored":
        return rtx.Scene(16, 12, MIRRORED, np.ones((2, 3), F), samples, leaf_max=1, **kw), MIRRORED
    raise KeyError(name)


def cull_delta(coords, created_eye):
    """PreparedScene::cull_delta, in f32: 2^-19 x the largest coordinate magnitude of the primitives' boxes and the eye"""
    magnitude = max(F(np.abs(np.asarray(coords, F)).max()), F(np.abs(np.asarray(created_eye, F)).max()))
    return F(F(magnitude) * F(2.0 ** -19)) + F(2.0 ** -100)


def bound_of(delta):
    """the largest |eye coordinate| rtx_render_view_rows accepts"""
    return F(F(delta) * F(2.0 ** 19))


def eyes(name, delta):
    """the scene's own eye, view_sets' side and back eyes, an eye on the bound (and, for the mirrored pair, one on x = 0)"""
    b = float(bound_of(delta))
    out = [CREATED_EYE[name], vs.BUNNY_VIEWS["side"][1], vs.BUNNY_VIEWS["back"][1], (-b, 0.25 * b, b)]
    if name == "mirrored":
        out.append((0.0, -7.0, 2.5))
    return out


def tree_root(nodes, n_global):
    return 2 if n_global and len(nodes) > 2 else 0


def dist2(lo, hi, eye):
    d2 = np.float64(0.0)
    for k in range(3):
        c = np.float64(0.5) * np.float64(lo[k]) + np.float64(0.5) * np.float64(hi[k]) - np.float64(F(eye[k]))
        d2 = d2 + c * c
    return d2


def restate(nodes, n_global, eye, delta):
    """nodes: uint32 [n, 8] as rtx_scene_nodes gives them (bmin xyz, link, bmax xyz, info).
    -> (the aimed stream in the same word order, inner nodes whose children were swapped, kept, tied)"""
    n = len(nodes)
    moved = nodes.copy()
    f = moved.view(F)
    f[:, 0:3] = nodes.view(F)[:, 0:3] - F(delta)
    f[:, 4:7] = nodes.view(F)[:, 4:7] + F(delta)
    root = tree_root(nodes, n_global)
    out = [moved[i].copy() for i in range(root)]
    count = dict(swapped=0, kept=0, tied=0)

    def visit(i):
        pos = len(out)
        out.append(moved[i].copy())
        if moved[i, 7] & LEAF:
            return
        a, b = i + 1, int(moved[i, 7])
        da, db = dist2(f[a, 0:3], f[a, 4:7], eye), dist2(f[b, 0:3], f[b, 4:7], eye)
        count["tied"] += int(da == db)
        first, second = (b, a) if db < da else (a, b)
        count["swapped" if first == b else "kept"] += 1
        visit(first)
        out[pos][7] = len(out)                 # info: the child visited second
        visit(second)
        out[pos][3] = len(out)                 # link: the record behind the subtree
    if root < n:
        visit(root)
    out = np.array(out, np.uint32).reshape(-1, 8)
    if root != 0:
        out[0, 3] = len(out)
    return out, count["swapped"], count["kept"], count["tied"]


def check_preorder(stream, root, leaves_of_input):
    """every inner node below root is followed by its first child, names its second child behind the first one's subtree
    and links behind both; the walk meets every record once; the leaves are the input's"""
    n = len(stream)

    def size(i, depth=0):
        assert i < n and depth <= 66
        if stream[i, 7] & LEAF:
            return 1
        first = size(i + 1, depth + 1)
        assert stream[i, 7] == i + 1 + first, i
        second = size(int(stream[i, 7]), depth + 1)
        assert stream[i, 3] == i + 1 + first + second, i
        return 1 + first + second
    assert root + size(root) == n
    below = stream[root:]
    leaves = below[(below[:, 7] & LEAF) != 0]
    assert sorted(map(tuple, leaves[:, [7, 3]].tolist())) == leaves_of_input
