"""Fixtures for the tests of a scene whose sample table is replaced (rtx_scene_resample, rtx_scene_reseed), with the CPU
oracle's answers: numpy, the oracle binding and the library's host side only, no GPU.

The expected value of every call on a resampled scene is the same call's on an ORACLE SCENE CREATED WITH THE NEW TABLE.

Two scenes, both created with table A (the first 4,096 pairs of the seeded table):
    yard    prims_sets' yard — 41 triangles, 5 spheres, two rays per pixel, ten light samples — created 24 x 16 with the
            yard view's camera, so that the calls that render the scene's own frame (rows, frame, tiles) see the yard too
    bunny   big_bunny + ground, 48 x 32 through lit_rows_sets' side view, one ray per pixel, 100 light samples, with the
            reference tree; its fixture light is light_sets' "far_side"

The tables (tables()).  A scene reads its table at the light indices (r * nb_ray + i) % n — the yard's are 0 .. 11 — and, for
the jitter of its primary rays, everywhere else too:
    B        equals A at every light index of the yard and differs at every other pair: only the jitter changes
    C        differs from A at the yard's light indices only: only the light points change
    D7, D1   7 pairs and 1 pair: fewer than a frame's pixels and than the light samples, so every modulus wraps
    Dbig     5,003 pairs: more than A, so a device's table buffer grows
    seed_*   rtxh_gen_samples(seed, 4,099) for SEEDS: an odd count, whose last pair is the kernel's 8-byte tail
    half     const_samples(0.5)
    inf      A with an infinite entry at a light index.  rtx_scene_create ACCEPTS it (the shaft margin folds the finite box
             words only), so rtx_scene_resample accepts it: the host tests pin the two to each other; no frame is rendered
tests/test_resample_sets.py asserts, without a GPU, that every table changes the frame; tests/test_resample_host.py and
tests/test_gpu_resample.py use them.  Everything is built once per process (query_sets._once)."""
import os

import numpy as np

import light_sets as ls
import lit_rows_sets as lr
import moves_sets as mv
import prims_sets as pm
import query_sets as qs
import shade_sets as ss
import skin_sets as sk
import view_sets as vs
from query_sets import F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_A = 4096
SEEDS = (0, 1, 2 ** 64 - 1, 20261020)
SEEDED_PAIRS = 4099
GROWN_PAIRS = 5003
WHOLE_PAIRS = 2000000
KERNEL_PAIRS = (1, 2, 3, 127, 128, 129, 511, 512, 513, 4099)
RENDERED = ("B", "C", "D7", "D1", "Dbig", "seed_0", "seed_1", "seed_max", "seed_more", "half")
SEED_OF = dict(seed_0=SEEDS[0], seed_1=SEEDS[1], seed_max=SEEDS[2], seed_more=SEEDS[3])
YARD_FRAME = pm.YARD_VIEW[0]
BUNNY_VIEW = lr.SIDE
BUNNY_LIGHT = ls.SIDE_LIGHTS["far_side"]
BUNNY_TABLES = ("B", "D7", "seed_1")
YARD_LIGHT = pm.POSE_LIGHT
POSES = (("prims", "all"), ("moved", "turn"), ("skinned", "bend"))


def light_indices(n, nb_ray=pm.NB_RAY, nb_light=pm.NB_LIGHT):
    return sorted({(r * nb_ray + i) % n for r in range(nb_ray) for i in range(nb_light)})


def tables(orc):
    def make():
        a = np.ascontiguousarray(orc.gen_samples()[:N_A])
        other = orc.gen_samples(777, N_A)
        at = light_indices(N_A)
        out = dict(A=a, B=other.copy(), C=a.copy(), D7=np.ascontiguousarray(other[100:107]), D1=np.array([[0.3125, 0.6875]], F),
                   Dbig=orc.gen_samples(779, GROWN_PAIRS), half=orc.const_samples(0.5, N_A), inf=a.copy())
        out["B"][at] = a[at]
        out["C"][at] = other[at]
        out["inf"][3, 0] = np.inf
        for name, seed in SEED_OF.items():
            out[name] = orc.gen_samples(seed, SEEDED_PAIRS)
        for t in out.values():
            t.setflags(write=False)
        return out
    return qs._once("resample_tables", make)


def apply(scene, orc, name):
    """puts table `name` into the library's scene the way the fixture is meant: seeded ones by the seed"""
    if name in SEED_OF:
        scene.reseed(SEED_OF[name], SEEDED_PAIRS)
    else:
        scene.resample(tables(orc)[name])


# ---------------------------------------------------------------------------------------------- the yard
def yard_kw(rtx_or_orc_kinds, **kw):
    return dict(dict(nb_ray=pm.NB_RAY, nb_light_sample=pm.NB_LIGHT, kinds=rtx_or_orc_kinds, **vs.camera(pm.YARD_VIEW)), **kw)


def open_yard(rtx, table, **kw):
    """the library's yard, created with its own frame and `table`"""
    y = pm.yard(rtx)
    more = dict(dict(reference_tree=rtx.REFTREE_NEVER, tie_rank=None), **kw)
    return rtx.Scene(YARD_FRAME[0], YARD_FRAME[1], y["tris"], y["rgb"], table, spheres=y["spheres"], sphere_rgb=y["sphere_rgb"],
                     **yard_kw(y["kinds"], **more))


def yard_oracle(orc, prims, table, **kw):
    return orc.Scene(YARD_FRAME[0], YARD_FRAME[1], prims["tris"], prims["rgb"], table, spheres=prims["spheres"],
                     sphere_rgb=prims["sphere_rgb"], **yard_kw(pm.kinds(), **kw))


def posed_prims(rtx, samples, pose):
    """the primitives of POSES' entry, every array in full"""
    kind, name = pose
    if kind == "prims":
        return pm.yard_pose(rtx, name)
    return mv.stated(rtx, samples, name) if kind == "moved" else sk.stated(rtx, samples, name)


def yard_render(orc, rtx, samples, table_name, pose=None, light=None):
    """the oracle scene of the yard (or of a pose's primitives) created with the table (and the light): dict(frame, stats,
    tri, lin, and — unposed, unlit — rays = (origins, directions) of the frame's primary rays as that scene makes them)"""
    def make():
        prims = pm.yard(rtx) if pose is None else posed_prims(rtx, samples, pose)
        t = tables(orc)[table_name]
        kw = {} if light is None else dict(light_tri=light[0], nb_light_sample=light[1] or pm.NB_LIGHT)
        osc = yard_oracle(orc, prims, t, **kw)
        frame, st, tri, lin = osc.render_rows(mode=orc.MODE_BVH, want_tri=True, want_lin=True)
        osc.close()
        out = dict(frame=frame, stats=st, tri=tri, lin=lin)
        if pose is None and light is None:
            (w, h), eye, look_at, distance = pm.YARD_VIEW
            o, d, _, _, _ = ss.camera_raw_rays(orc, w, h, eye, look_at, vs.UP, distance, t, pm.NB_RAY)
            out["rays"] = (o, d)
        for a in (frame, tri, lin):
            a.setflags(write=False)
        return out
    return qs._once("resample_yard_%s_%s_%s" % (table_name, pose, light is not None), make)


def yard_queries(orc, rtx, samples):
    """rays into the yard and their answers, which no table changes: prims_sets.query_set of the identity pose"""
    return pm.query_set(orc, rtx, samples, "identity")


# ---------------------------------------------------------------------------------------------- the bunny
def bunny_kw():
    return vs.camera(BUNNY_VIEW)


def open_bunny(rtx, table):
    return rtx.default_scene([os.path.join(ROOT, "models", "big_bunny.obj")], BUNNY_VIEW[0][0], BUNNY_VIEW[0][1], table, **bunny_kw())


def bunny_render(orc, table_name, lit=False):
    def make():
        kw = dict(light_tri=BUNNY_LIGHT[0], nb_light_sample=BUNNY_LIGHT[1]) if lit else {}
        osc = orc.default_scene(["big_bunny.obj"], BUNNY_VIEW[0][0], BUNNY_VIEW[0][1], tables(orc)[table_name], **dict(bunny_kw(), **kw))
        frame, st = osc.render_rows(mode=orc.MODE_BVH)
        osc.close()
        frame.setflags(write=False)
        return dict(frame=frame, stats=st)
    return qs._once("resample_bunny_%s_%s" % (table_name, lit), make)


# ---------------------------------------------------------------------------------------------- the statement in numpy
def stated(seed, first, count):
    """pairs [first, first + count) of the seeded table by sample_statement's closed form, in 64-bit integer arithmetic"""
    i = (2 * first + np.arange(2 * count, dtype=np.uint64)).astype(np.uint64)
    with np.errstate(over="ignore"):
        z = np.uint64(seed) + (i + np.uint64(1)) * np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
    return ((z >> np.uint64(40)).astype(np.uint32).astype(F) * F(2.0 ** -24)).reshape(count, 2)
