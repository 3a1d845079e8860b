"""The pose path as a whole (rtx_scene_pose, _rebuilt, _prims, _moved, _skinned and their _device twins): the ten entry
points share one set of library-owned buffers per device, one launch sequence and one family of refusals.

1. The five families take turns on one yard and one stream, in an order in which every shared buffer holds another family's
   leftovers when a call arrives.  After every call the pose the device holds is compared word for word with the host
   statement of what the call stated, and rtx_debug_moved_prims answers exactly while the move or skin kernel was the last
   writer of the two arrays it reads.
2. Every refusal of every entry point, alone and in pairs, with the code it is refused with.  The calls are made on the
   exported functions (Scene methods cannot state a NULL struct, an unknown flag bit or a group on a skinned call), with
   the binding's own structs.  After every refused call the pose that stood before reads back unchanged.

Every comparison is for equal words."""
import ctypes as C
import importlib
import itertools

import numpy as np
import pytest

import moves_sets as mv
import prims_sets as pm
import skin_sets as sk
from query_sets import F, bits

pytestmark = pytest.mark.gpu

EYE = (30.0, 120.0, 250.0)
BAD_ARG, UNSUPPORTED = -1, -5


@pytest.fixture(scope="module")
def rtx():
    mod = importlib.import_module("ray-tracer-rust_amd")
    assert mod.device_count() >= 1, "no HIP device: the product path has no CPU fallback"
    assert (mod.ERR_BAD_ARG, mod.ERR_UNSUPPORTED) == (BAD_ARG, UNSUPPORTED)
    return mod


def same_words(got, want, what):
    for g, w, part in zip(got, want, ("primitive", "shading", "node")):
        bad = np.argwhere(g != w)
        assert not len(bad), "%s: %s words differ at %s" % (what, part, bad[:6].tolist())


def device_array(torch, a):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).to("cuda:0")


# ---------------------------------------------------------------------------------------------- 1: the families take turns
def stated_by(scene, family, kw):
    """what a call of `family` with keywords `kw` states, as keywords of pose_prims_records (None: as uploaded), and the
    arrays the move or skin kernel writes for it (None: the family runs neither)"""
    if family == "vertices":
        return dict(v0v1v2=kw["v0v1v2"], spheres=None, rgb=None, sphere_rgb=None), None
    if family == "prims":
        return dict(kw), None
    if family == "moved":
        v, s = scene.moved_prims(**mv.statement_kw(kw))
    else:
        v, s = scene.skinned_prims(**sk.statement_kw(kw))
    return dict(v0v1v2=v, spheres=s, rgb=kw["rgb"], sphere_rgb=kw["sphere_rgb"]), (v, s)


def test_the_five_families_take_turns_on_one_yard_and_one_stream(rtx, samples_seeded):
    torch = pytest.importorskip("torch")
    y = pm.yard(rtx)
    turned = {d: pm.turned(y["tris"], d) for d in (25.0, -15.0, 60.0, 100.0)}
    rank = np.arange(pm.N_PRIMS, dtype=np.uint32)[::-1].copy()
    prims = dict(all=pm.given(rtx, "all"), recolour=pm.given(rtx, "recolour"), move=pm.given(rtx, "move"),
                 bare=dict(v0v1v2=turned[60.0], spheres=None, rgb=None, sphere_rgb=None))
    moved = {n: mv.moves(rtx, n) for n in ("all", "turn", "balls", "shear")}
    s_all = sk.moves(rtx, "all")
    swapped = s_all["moves"].copy()
    swapped[[0, 1]] = swapped[[1, 0]]
    skinned = dict(all=s_all, swapped=dict(s_all, moves=swapped, rgb=None, sphere_rgb=None),
                   unscaled=dict(s_all, radius_scale=None, sphere_rgb=None))
    # (family, keywords, host or device form, rebuilt, tie_rank given)
    turns = [("vertices", dict(v0v1v2=turned[25.0]), "host", False, False),
             ("skinned", skinned["all"], "device", False, False),
             ("prims", prims["all"], "host", False, False),                  # spheres stated: the host's copy of them
             ("moved", moved["all"], "device", True, False),
             ("vertices", dict(v0v1v2=turned[-15.0]), "host", True, True),
             ("prims", prims["recolour"], "device", False, False),           # no spheres stated
             ("skinned", skinned["swapped"], "host", True, False),
             ("vertices", dict(v0v1v2=turned[60.0]), "device", False, False),
             ("moved", moved["turn"], "host", False, True),
             ("prims", prims["all"], "device", True, True),
             ("skinned", skinned["unscaled"], "device", True, False),
             ("vertices", dict(v0v1v2=turned[100.0]), "device", True, True),
             ("moved", moved["balls"], "device", False, False),
             ("prims", prims["recolour"], "host", True, False),
             ("skinned", skinned["all"], "host", False, True),
             ("moved", moved["shear"], "host", True, False),
             ("prims", prims["bare"], "host", False, False),                 # nothing stated beside the vertices
             ("vertices", dict(v0v1v2=turned[25.0]), "device", False, False),
             ("prims", prims["move"], "device", False, False),               # the caller's spheres, none of the library's
             ("skinned", skinned["swapped"], "device", False, True),
             ("prims", prims["move"], "host", True, True)]
    seen = {(f, form, r) for f, _, form, r, _ in turns}
    assert seen == set(itertools.product(("vertices", "prims", "moved", "skinned"), ("host", "device"), (False, True)))
    names = dict(v0v1v2="d_v0v1v2_ptr", spheres="d_spheres_ptr", moves="d_moves_ptr", group="d_group_ptr",
                 radius_scale="d_radius_scale_ptr", rgb="d_rgb_ptr", sphere_rgb="d_sphere_rgb_ptr")
    keep = []

    def on_device(kw):
        out = {}
        for k, a in kw.items():
            if a is not None:
                keep.append(device_array(torch, a))
                out[names[k]] = keep[-1].data_ptr()
        return out

    d_turns = [on_device(kw) if form == "device" else None for _, kw, form, _, _ in turns]
    d_rank = device_array(torch, rank)
    torch.cuda.synchronize()
    stream = torch.cuda.Stream(device="cuda:0")
    assert stream.cuda_stream != torch.cuda.default_stream().cuda_stream
    with pm.open_yard(rtx, samples_seeded) as scene:
        assert scene.info()["n_global"] >= 1 and len(scene.spheres) >= 2 and scene.primary_nodes()[1]
        scene.skin(**sk.skin(rtx, "all"))
        arrays = None               # the model: what the move or skin kernel wrote, until a host copy overwrites it
        for k, (family, kw, form, rebuilt, ranked) in enumerate(turns):
            what = "turn %d: %s, %s form, %s" % (k, family, form, "rebuilt" if rebuilt else "refitted")
            given, made = stated_by(scene, family, kw)
            if form == "host":
                tr = dict(tie_rank=rank if ranked else None)
                if family == "vertices":
                    (scene.pose_rebuilt if rebuilt else scene.pose)(kw["v0v1v2"], **tr)
                else:
                    dict(prims=scene.pose_prims, moved=scene.pose_moved, skinned=scene.pose_skinned)[family](rebuilt=rebuilt, **tr, **kw)
                arrays = made       # (None: the copies overwrote the arrays)
            else:
                d = dict(d_turns[k], d_tie_rank_ptr=d_rank.data_ptr() if ranked else None, stream=stream.cuda_stream)
                if family == "vertices":
                    (scene.pose_rebuilt_device if rebuilt else scene.pose_device)(0, **d)
                elif family == "prims":
                    scene.pose_prims_device(0, rebuilt=rebuilt, **d)
                elif family == "moved":
                    scene.pose_moved_device(0, n_moves=len(kw["moves"]), rebuilt=rebuilt, **d)
                else:
                    scene.pose_skinned_device(0, n_moves=len(kw["moves"]), rebuilt=rebuilt, **d)
                if made is not None:
                    arrays = made   # (the caller's own vertices and spheres are read where they lie: nothing overwritten)
            # the read-backs drain the caller's stream: nothing else waits for the call
            tr = rank if ranked else None
            if rebuilt:
                if family == "vertices":
                    _, perm, t, s, n = scene.rebuilt_records(kw["v0v1v2"], tie_rank=tr)
                    aimed = scene.rebuilt_aimed(kw["v0v1v2"], EYE)
                else:
                    _, perm, t, s, n = scene.pose_prims_records(rebuilt=True, tie_rank=tr, **given)
                    aimed = scene.pose_prims_aimed(EYE, rebuilt=True, **given)
                dperm, dt, ds, dn, daimed = scene.debug_pose_rebuilt(EYE)
                assert np.array_equal(dperm, perm), what + ": permutation"
                same_words((dt, ds, dn), (t, s, n), what)
                assert np.array_equal(daimed, aimed), what + ": the aimed stream"
                with pytest.raises(rtx.RtxError) as e:                  # sized by the uploaded node count
                    scene.debug_pose()
                assert e.value.code == BAD_ARG, what
            else:
                want = scene.posed_records(kw["v0v1v2"], tie_rank=tr) if family == "vertices" else \
                    scene.pose_prims_records(tie_rank=tr, **given)
                same_words(scene.debug_pose(), want, what)
                with pytest.raises(rtx.RtxError) as e:
                    scene.debug_pose_rebuilt(EYE)
                assert e.value.code == BAD_ARG, what
            if arrays is None:
                with pytest.raises(rtx.RtxError) as e:
                    scene.debug_moved_prims()
                assert e.value.code == BAD_ARG, what
            else:
                for g, w, part in zip(scene.debug_moved_prims(), arrays, ("vertex", "sphere")):
                    assert np.array_equal(bits(g), bits(w)), "%s: the kernel's %s array" % (what, part)
        stream.synchronize()


# ---------------------------------------------------------------------------------------------- 2: every refusal, in order
# Per entry point the faults in the order the library looks for them, each with the code it is refused with.  A call with
# two of them is refused with the code of the one that stands first.  (Faults refused with the same code cannot be told
# apart from outside: among those the order is the source's, and nothing here depends on it.)
VERTICES_HOST = [("null scene", BAD_ARG), ("null vertices", BAD_ARG), ("reference_tree 3", BAD_ARG), ("far vertices", UNSUPPORTED)]
VERTICES_DEVICE = [("null scene", BAD_ARG), ("null vertices", BAD_ARG), ("misaligned v", BAD_ARG), ("misaligned rank", BAD_ARG)]
MOVES_HEAD = [("null scene", BAD_ARG), ("null struct", BAD_ARG), ("unknown flag", BAD_ARG)]
COUNTS = [("null moves", BAD_ARG), ("n_moves 0", BAD_ARG), ("n_moves 65537", BAD_ARG)]
REFUSALS = {
    "rtx_scene_pose": VERTICES_HOST,
    "rtx_scene_pose_rebuilt": VERTICES_HOST,
    "rtx_scene_pose_device": VERTICES_DEVICE,
    "rtx_scene_pose_rebuilt_device": VERTICES_DEVICE,
    "rtx_scene_pose_prims": MOVES_HEAD + [("null vertices", BAD_ARG), ("reference_tree 3", BAD_ARG), ("far vertices", UNSUPPORTED),
                                          ("far spheres", UNSUPPORTED)],
    "rtx_scene_pose_prims_device": MOVES_HEAD + [("null vertices", BAD_ARG), ("misaligned v", BAD_ARG), ("misaligned rank", BAD_ARG),
                                                 ("misaligned spheres", BAD_ARG), ("misaligned rgb", BAD_ARG),
                                                 ("misaligned sphere_rgb", BAD_ARG)],
    "rtx_scene_pose_moved": MOVES_HEAD + [("reference_tree 3", BAD_ARG)] + COUNTS + [("group of n_moves", BAD_ARG),
                                                                                   ("far moves", UNSUPPORTED)],
    "rtx_scene_pose_moved_device": MOVES_HEAD + COUNTS + [("misaligned rank", BAD_ARG), ("misaligned rgb", BAD_ARG),
                                                          ("misaligned sphere_rgb", BAD_ARG), ("misaligned moves", BAD_ARG),
                                                          ("misaligned group", BAD_ARG), ("misaligned radius_scale", BAD_ARG)],
    "rtx_scene_pose_skinned": MOVES_HEAD + [("reference_tree 3", BAD_ARG)] + COUNTS + [("a group", BAD_ARG), ("no skin", BAD_ARG),
                                                                                     ("n_moves 3 <= bone 6", BAD_ARG),
                                                                                     ("far moves", UNSUPPORTED)],
    "rtx_scene_pose_skinned_device": MOVES_HEAD + COUNTS + [("a group", BAD_ARG), ("no skin", BAD_ARG), ("misaligned rank", BAD_ARG),
                                                            ("misaligned rgb", BAD_ARG), ("misaligned sphere_rgb", BAD_ARG),
                                                            ("misaligned moves", BAD_ARG), ("misaligned radius_scale", BAD_ARG)],
}
# the argument a fault changes (two faults of one argument are not combined)
ARGUMENT = {"null scene": "scene", "no skin": "scene", "null struct": "struct", "unknown flag": "flags", "reference_tree 3": "ref",
            "null vertices": "v", "far vertices": "v", "misaligned v": "v", "far spheres": "spheres", "misaligned spheres": "spheres",
            "null moves": "moves", "far moves": "moves", "misaligned moves": "moves", "n_moves 0": "n_moves",
            "n_moves 65537": "n_moves", "n_moves 3 <= bone 6": "n_moves", "a group": "group", "group of n_moves": "group",
            "misaligned group": "group", "misaligned rank": "rank", "misaligned rgb": "rgb", "misaligned sphere_rgb": "sphere_rgb",
            "misaligned radius_scale": "radius_scale"}


def addr(a):
    """the address of a numpy array, an address as it is, None: NULL"""
    return a.ctypes.data if isinstance(a, np.ndarray) else a


def call(rtx, name, a):
    """the exported function `name` on the arguments `a`"""
    lib, m = rtx.rtx._lib, rtx.rtx
    host = not name.endswith("_device")
    tail = (a["ref"], None) if host else (None,)                       # reference_tree and stats, or the stream: NULL
    h = a["scene"].handle if a["scene"] is not None else None
    if "prims" in name:
        st = m.RtxPosePrims(*[addr(a[k]) for k in ("v", "spheres", "rgb", "sphere_rgb", "rank")])
    elif "moved" in name or "skinned" in name:
        st = m.RtxPoseMoves(a["n_moves"], *[addr(a[k]) for k in ("moves", "group", "radius_scale", "rgb", "sphere_rgb", "rank")])
    else:
        v, rank = addr(a["v"]), addr(a["rank"])
        if host:
            return getattr(lib, name)(h, 0, C.cast(v, m.f32p), C.cast(rank, m.u32p), *tail)
        return getattr(lib, name)(h, 0, v, rank, *tail)
    return getattr(lib, name)(h, 0, C.byref(st) if a["struct"] else None, a["flags"], *tail)


def test_every_refusal_and_the_order_of_two(rtx, samples_seeded):
    torch = pytest.importorskip("torch")
    y = pm.yard(rtx)
    kw = sk.moves(rtx, "all")
    n_moves = len(kw["moves"])
    assert n_moves == 7
    rank = np.arange(pm.N_PRIMS, dtype=np.uint32)[::-1].copy()
    group = np.full(pm.N_PRIMS, mv.NONE, np.uint32)
    with pm.open_yard(rtx, samples_seeded) as scene, pm.open_yard(rtx, samples_seeded) as bare, \
            pm.open_sized(rtx, samples_seeded, pm.size_scenes(rtx)["spheres_only"]) as balls:
        bound = float(scene.pose_bound())
        scene.skin(**sk.skin(rtx, "all"))
        assert scene.skin_bound() == (True, 6) and bare.skin_bound()[0] is False
        far_v, far_s, far_m, wild = y["tris"].copy(), y["spheres"].copy(), kw["moves"].copy(), group.copy()
        far_v[40, 4], far_s[3, 2], far_m[0, 7], wild[5] = 2.0 * bound, -2.0 * bound, 4.0 * bound, n_moves
        host = dict(v=y["tris"].copy(), spheres=y["spheres"].copy(), rgb=y["rgb"].copy(), sphere_rgb=y["sphere_rgb"].copy(), rank=rank,
                    moves=kw["moves"], group=None, radius_scale=kw["radius_scale"])
        keep = {k: device_array(torch, a) for k, a in dict(host, group=group).items()}
        torch.cuda.synchronize()
        device = {k: t.data_ptr() for k, t in keep.items()}
        faults = {"null scene": None, "no skin": bare, "null struct": False, "unknown flag": 2, "reference_tree 3": 3, "null vertices": None,
                  "far vertices": far_v, "far spheres": far_s, "null moves": None, "far moves": far_m, "n_moves 0": 0,
                  "n_moves 65537": 65537, "n_moves 3 <= bone 6": 3, "a group": group, "group of n_moves": wild}
        # the poses that stand while the calls are refused: a moved one on the yard, a rebuilt one on the scene without a skin
        scene.pose_moved(**mv.moves(rtx, "all"))
        bare.pose_rebuilt(pm.turned(y["tris"], 25.0))
        standing = scene.debug_pose(), scene.debug_moved_prims(), bare.debug_pose_rebuilt(EYE)

        def still_standing(what):
            same_words(scene.debug_pose(), standing[0], what + ": the yard's pose afterwards")
            assert all(np.array_equal(bits(g), bits(w)) for g, w in zip(scene.debug_moved_prims(), standing[1])), what
            assert all(np.array_equal(g, w) for g, w in zip(bare.debug_pose_rebuilt(EYE), standing[2])), what

        n_calls = 0
        for name, order in REFUSALS.items():
            on_host = not name.endswith("_device")
            base = dict(host if on_host else dict(device, group=None), scene=scene, struct=True, flags=0, ref=rtx.REFTREE_NEVER,
                        n_moves=n_moves)
            if "skinned" not in name and not on_host:
                base["group"] = device["group"]
            sets = [(f,) for f, _ in order] + [p for p in itertools.combinations([f for f, _ in order], 2)
                                               if ARGUMENT[p[0]] != ARGUMENT[p[1]]]
            for fs in sets:
                a = dict(base)
                for f in fs:
                    if f.startswith("misaligned"):
                        a[ARGUMENT[f]] = device["group" if f == "misaligned group" else ARGUMENT[f]] + 2
                    elif f == "a group" and not on_host:
                        a["group"] = device["group"]
                    else:
                        a[ARGUMENT[f]] = faults[f]
                want = dict(order)[min(fs, key=[f for f, _ in order].index)]
                got = call(rtx, name, a)
                assert got == want, "%s with %s: refused with %d, not with %d" % (name, " and ".join(fs), got, want)
                still_standing("%s with %s" % (name, " and ".join(fs)))
                n_calls += 1
        assert n_calls > 200
        # NULL vertices on a scene without triangles: the vertex entry points refuse them, rtx_scene_pose_prims reads none
        sp = pm.size_scenes(rtx)["spheres_only"]["pose"]["spheres"]
        d_sp = device_array(torch, sp)
        torch.cuda.synchronize()
        none = dict(scene=balls, v=None, rank=None, rgb=None, sphere_rgb=None, struct=True, flags=0, ref=rtx.REFTREE_NEVER)
        for name in ("rtx_scene_pose", "rtx_scene_pose_rebuilt", "rtx_scene_pose_device", "rtx_scene_pose_rebuilt_device"):
            assert call(rtx, name, none) == BAD_ARG, name
        want = balls.pose_prims_records(spheres=sp)
        assert call(rtx, "rtx_scene_pose_prims", dict(none, spheres=sp)) == 0
        same_words(balls.debug_pose(), want, "NULL vertices, no triangles, host form")
        balls.pose_prims(spheres=pm.size_scenes(rtx)["spheres_only"]["spheres"])
        assert call(rtx, "rtx_scene_pose_prims_device", dict(none, spheres=d_sp.data_ptr())) == 0
        same_words(balls.debug_pose(), want, "NULL vertices, no triangles, device form")
        assert call(rtx, "rtx_scene_pose_prims", dict(none, spheres=sp, ref=3)) == BAD_ARG
        torch.cuda.synchronize()
