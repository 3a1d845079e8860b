"""A model of a live scene for randomised sequences of the calls that change one without creating a new one — the five
kinds of pose, a bound skin, a replaced or reseeded sample table — and of the calls that observe it under the scene's or
another light: numpy only, no pytest, no GPU, and never the library's host statements.

    random_scene    the stress test's draw, kept bit for bit (tests/test_gpu_stress.py imports it back)
    FAMILY          twelve scenes of that distribution (frame at most 32 x 24, 1 / 7 / 32 light samples, one or two rays, a
                    4096-pair table) whose primitive counts are pinned to the wavefront and workgroup edges of the move,
                    skin, overlay and rebuild kernels; the seeds were chosen on the CPU so that the oracle's frame of each
                    scene's own view has at least 100 primary hits and no non-finite hit distance
                    (tests/test_sequence_model.py asserts it)
    Model           what the library must hold: the scene as created, the current table (an array, or seed and pairs), the
                    bound skin, per device the standing pose — the stated arrays in full and the `rebuilt` flag
    draw_log        a seeded log of operations — state changes, refused calls, observations — every one kept inside the
                    contract by the model (the range rule; no direction with a zero component); a draw that leaves it is
                    redrawn at most 8 times, then the step becomes an observation
    Expect          the oracle's answer for an observation, from a fresh oracle scene created with the model's primitives,
                    table and light and the observation's camera, cached by state
    coverage        the transitions a log holds, for tests/test_sequence_model.py's table

A log depends on (scene, seed, steps, devices) only: RTX_SEQUENCE_SEED and RTX_SEQUENCE_STEPS replay or lengthen it."""
import hashlib
import os

import numpy as np

import moves_sets as mv
import np_ref
import query_sets as qs
import resample_sets as rs
import shade_sets as ss
import skin_sets as sk

F = np.float32
NONE = 0xFFFFFFFF
UP = (0.0, 1.0, 0.0)
OK, ERR_BAD_ARG, ERR_UNSUPPORTED = 0, -1, -5
ACCEL_BVH, ACCEL_BRUTE = 0, 1
# the smallest number of steps per sequence at which every cap and every line of the coverage table holds over the twelve
# sequences (tests/test_sequence_model.py); RTX_SEQUENCE_STEPS lengthens it for a soak
STEPS = 40
BASE_SEED = 20261021
POSE_KINDS = ("pose", "pose_rebuilt", "pose_prims", "pose_moved", "pose_skinned")
REFUSALS = ("skinned_without_skin", "skinned_with_group", "skinned_few_moves", "moved_out_of_bound", "posed_without_pose",
            "bad_group", "resample_nothing")
LIGHT_COUNTS = (0, 1, 7, 32, 100, 130)
BATCHES = (1, 63, 64, 65, 200)
TABLE_PAIRS = (1, 3, 4096, 5003)
SEED_PAIRS = (1, 129, 4099)
REDRAWS = 8


def random_scene(rng):
    n_tris = int(rng.integers(1, 400))
    scale = float(10.0 ** rng.uniform(-1.0, 3.0))               # scene extent from 0.1 to 1000 units
    centre = rng.uniform(-1.0, 1.0, 3) * scale * float(rng.choice([0.0, 1.0, 30.0]))
    c = rng.uniform(-1.0, 1.0, size=(n_tris, 1, 3)) * scale
    size = scale * float(10.0 ** rng.uniform(-2.0, 0.0))
    v = (centre + c + rng.uniform(-1.0, 1.0, size=(n_tris, 3, 3)) * size).astype(F)
    tris = v.reshape(-1, 9)
    rgb = rng.uniform(0.0, 1.0, size=(n_tris, 3)).astype(F)
    if rng.random() < 0.5:                                      # grey scene: the one-channel accumulation path
        rgb[:] = rgb[:, :1]
    if rng.random() < 0.6:                                      # a floor spanning the scene: a "global" triangle
        y = float(centre[1] - 1.2 * scale)
        floor = np.array([[centre[0] - 40 * scale, y, centre[2] - 40 * scale, centre[0] + 40 * scale, y,
                           centre[2] - 40 * scale, centre[0], y, centre[2] + 40 * scale]], F)
        tris = np.concatenate([tris, floor])
        rgb = np.concatenate([rgb, np.array([[0.5, 0.5, 0.5]], F)])
    n_sph = int(rng.integers(0, 30)) if rng.random() < 0.4 else 0
    spheres = np.concatenate([centre + rng.uniform(-1.0, 1.0, size=(n_sph, 3)) * scale,
                              rng.uniform(0.02, 0.3, size=(n_sph, 1)) * scale], axis=1).astype(F)
    srgb = rng.uniform(0.0, 1.0, size=(n_sph, 3)).astype(F)
    kinds = np.zeros(len(tris) + n_sph, np.uint8)
    kinds[rng.choice(len(kinds), n_sph, replace=False)] = 1
    direction = rng.normal(size=3)
    eye = centre + direction / np.linalg.norm(direction) * scale * rng.uniform(1.5, 4.0)
    light_c = centre + np.array([rng.uniform(-1, 1), rng.uniform(1.5, 4.0), rng.uniform(-1, 1)]) * scale
    light = (light_c + rng.uniform(-0.1, 0.1, size=(3, 3)) * scale).astype(F).reshape(9)
    W, H = int(rng.integers(9, 70)), int(rng.integers(9, 70))
    kw = dict(eye=tuple(float(x) for x in eye.astype(F)), look_at=tuple(float(x) for x in centre.astype(F)),
              up=(0.0, 1.0, 0.0), distance=float(rng.uniform(0.6, 2.5) * max(W, H)),
              light_tri=tuple(float(x) for x in light), nb_ray=int(rng.choice([1, 1, 1, 2])),
              nb_light_sample=int(rng.choice([1, 7, 32, 100, 130])))
    return W, H, tris, rgb, spheres, srgb, kinds, kw


# ------------------------------------------------------------------------------------------------ the twelve scenes
# name, mesh triangles (the floor comes on top), floor, spheres, leaf_max, accel, the scene's seed
FAMILY = (
    dict(name="t1", n_tris=1, floor=True, n_sph=0, leaf_max=0, accel=ACCEL_BVH, seed=102),    # (its triangle covers 110 pixels)
    dict(name="t21_brute", n_tris=21, floor=False, n_sph=1, leaf_max=1, accel=ACCEL_BRUTE, seed=1108),
    dict(name="t22", n_tris=22, floor=True, n_sph=20, leaf_max=8, accel=ACCEL_BVH, seed=2100),
    dict(name="t63", n_tris=63, floor=False, n_sph=0, leaf_max=0, accel=ACCEL_BVH, seed=3107),
    dict(name="t64_no_global", n_tris=64, floor=False, n_sph=0, leaf_max=1, accel=ACCEL_BVH, seed=4104),
    dict(name="t65", n_tris=65, floor=True, n_sph=1, leaf_max=8, accel=ACCEL_BVH, seed=5100),
    dict(name="t85", n_tris=85, floor=True, n_sph=20, leaf_max=0, accel=ACCEL_BVH, seed=6101),
    dict(name="t86", n_tris=86, floor=False, n_sph=20, leaf_max=1, accel=ACCEL_BVH, seed=7100),
    dict(name="t255", n_tris=255, floor=True, n_sph=0, leaf_max=8, accel=ACCEL_BVH, seed=8100),
    dict(name="t256", n_tris=256, floor=False, n_sph=1, leaf_max=0, accel=ACCEL_BVH, seed=9101),
    dict(name="t257", n_tris=257, floor=True, n_sph=20, leaf_max=1, accel=ACCEL_BVH, seed=10100),
    dict(name="spheres_only", n_tris=0, floor=False, n_sph=20, leaf_max=0, accel=ACCEL_BVH, seed=11100),
)
NAMES = tuple(f["name"] for f in FAMILY)


def family_scene(spec):
    """random_scene's distribution with the counts of `spec` pinned, a frame of at most 32 x 24, 1 / 7 / 32 light samples
    and one or two rays per pixel -> dict(W, H, tris, rgb, spheres, srgb, kinds, kw, centre, scale, floor: the floor's
    triangle number or None)"""
    rng = np.random.default_rng(spec["seed"])
    n_tris, n_sph = spec["n_tris"], spec["n_sph"]
    scale = float(10.0 ** rng.uniform(-1.0, 3.0))
    centre = rng.uniform(-1.0, 1.0, 3) * scale * float(rng.choice([0.0, 1.0, 30.0]))
    c = rng.uniform(-1.0, 1.0, size=(n_tris, 1, 3)) * scale
    size = scale * float(10.0 ** rng.uniform(-2.0, 0.0))
    tris = (centre + c + rng.uniform(-1.0, 1.0, size=(n_tris, 3, 3)) * size).astype(F).reshape(-1, 9)
    rgb = rng.uniform(0.0, 1.0, size=(n_tris, 3)).astype(F)
    if rng.random() < 0.5:
        rgb[:] = rgb[:, :1]
    if spec["floor"]:
        y = float(centre[1] - 1.2 * scale)
        floor = np.array([[centre[0] - 40 * scale, y, centre[2] - 40 * scale, centre[0] + 40 * scale, y,
                           centre[2] - 40 * scale, centre[0], y, centre[2] + 40 * scale]], F)
        tris = np.concatenate([tris, floor])
        rgb = np.concatenate([rgb, np.array([[0.5, 0.5, 0.5]], F)])
    spheres = np.concatenate([centre + rng.uniform(-1.0, 1.0, size=(n_sph, 3)) * scale,
                              rng.uniform(0.02, 0.3, size=(n_sph, 1)) * scale], axis=1).astype(F)
    srgb = rng.uniform(0.0, 1.0, size=(n_sph, 3)).astype(F)
    kinds = np.zeros(len(tris) + n_sph, np.uint8)
    kinds[rng.choice(len(kinds), n_sph, replace=False)] = 1
    direction = rng.normal(size=3)
    eye = centre + direction / np.linalg.norm(direction) * scale * rng.uniform(1.5, 4.0)
    light_c = centre + np.array([rng.uniform(-1, 1), rng.uniform(1.5, 4.0), rng.uniform(-1, 1)]) * scale
    light = (light_c + rng.uniform(-0.1, 0.1, size=(3, 3)) * scale).astype(F).reshape(9)
    W, H = int(rng.integers(9, 33)), int(rng.integers(9, 25))
    kw = dict(eye=tuple(float(x) for x in eye.astype(F)), look_at=tuple(float(x) for x in centre.astype(F)), up=UP,
              distance=float(rng.uniform(0.6, 2.5) * max(W, H)), light_tri=tuple(float(x) for x in light),
              nb_ray=int(rng.choice([1, 2])), nb_light_sample=int(rng.choice([1, 7, 32])))
    return dict(W=W, H=H, tris=np.ascontiguousarray(tris), rgb=np.ascontiguousarray(rgb), spheres=spheres, srgb=srgb, kinds=kinds,
                kw=kw, centre=centre.astype(np.float64), scale=scale, floor=(len(tris) - 1 if spec["floor"] else None),
                leaf_max=spec["leaf_max"], accel=spec["accel"], name=spec["name"])


def created_prims(sc):
    return dict(tris=sc["tris"], spheres=sc["spheres"], rgb=sc["rgb"], sphere_rgb=sc["srgb"])


def open_scene(rtx, sc, table):
    """the library's scene of a family member (host only until a device is named)"""
    extra = dict(spheres=sc["spheres"], sphere_rgb=sc["srgb"], kinds=sc["kinds"]) if len(sc["spheres"]) else {}
    return rtx.Scene(sc["W"], sc["H"], sc["tris"], sc["rgb"], table, accel=sc["accel"], leaf_max=sc["leaf_max"], **extra, **sc["kw"])


def sphere_boxes(spheres):
    """origin -+ radius, each rounded to f32 once: the six box words the range rule reads"""
    s = np.asarray(spheres, F).reshape(-1, 4)
    return np.concatenate([(s[:, :3] - s[:, 3:4]).astype(F), (s[:, :3] + s[:, 3:4]).astype(F)], axis=1)


def digest(*parts):
    h = hashlib.sha1()
    for p in parts:
        h.update(np.ascontiguousarray(p).tobytes() if isinstance(p, np.ndarray) else repr(p).encode())
    return h.hexdigest()


# ------------------------------------------------------------------------------------------------ the model
class Model:
    def __init__(self, sc, table, n_devices=1):
        self.sc = sc
        self.created = created_prims(sc)
        self.table = np.ascontiguousarray(table, F)             # or ("seed", seed, n_pairs)
        self.skin = None                                        # dict(bones, weights, sphere_bone)
        self.pose = [None] * n_devices                          # dict(tris, spheres, rgb, sphere_rgb, rebuilt, kind, moved)
        boxes = np.concatenate([sc["tris"].reshape(-1), sphere_boxes(sc["spheres"]).reshape(-1), np.asarray(sc["kw"]["eye"], F)])
        self.bound = F(np.abs(boxes).max())                     # rtx_scene_pose_bound: box words and the created eye
        self.tri_at = np.nonzero(sc["kinds"] == 0)[0]           # Vec position of triangle n
        self.sphere_at = np.nonzero(sc["kinds"] != 0)[0]

    def table_array(self):
        if isinstance(self.table, tuple):
            return rs.stated(self.table[1], 0, self.table[2])
        return self.table

    def table_key(self):
        return self.table if isinstance(self.table, tuple) else digest(self.table)

    def max_bone(self):
        if self.skin is None:
            return 0
        b = np.concatenate([self.skin["bones"].reshape(-1), self.skin["sphere_bone"].reshape(-1)])
        b = b[b != NONE]
        return int(b.max()) if len(b) else 0

    def in_range(self, tris, spheres):
        w = np.concatenate([np.asarray(tris, F).reshape(-1), np.asarray(spheres, F).reshape(-1), sphere_boxes(spheres).reshape(-1)])
        return bool(np.isfinite(w).all() and (np.abs(w) <= self.bound).all())

    def stated(self, op):
        """the arrays a pose states, every one in full, by the suite's numpy restatements and plain copies"""
        c, kind = self.created, op["op"]
        if kind in ("pose", "pose_rebuilt"):
            tris, spheres = op["tris"], c["spheres"]
        elif kind == "pose_prims":
            tris, spheres = op["tris"], (c["spheres"] if op["spheres"] is None else op["spheres"])
        elif kind == "pose_moved":
            tris, spheres = mv.restated(c["tris"], c["spheres"], self.sc["kinds"], op["moves"], op["group"], op["radius_scale"])
        else:
            s = self.skin
            tris, spheres = sk.restated(c["tris"], c["spheres"], s["bones"], s["weights"], s["sphere_bone"], op["moves"], op["radius_scale"])
        rgb = c["rgb"] if op.get("rgb") is None else op["rgb"]
        srgb = c["sphere_rgb"] if op.get("sphere_rgb") is None else op["sphere_rgb"]
        return dict(tris=np.ascontiguousarray(tris, F).reshape(-1, 9), spheres=np.ascontiguousarray(spheres, F).reshape(-1, 4),
                    rgb=np.ascontiguousarray(rgb, F), sphere_rgb=np.ascontiguousarray(srgb, F))

    def apply(self, op):
        """a state change; a refused call and an observation change nothing"""
        kind = op["op"]
        if op.get("refused") or kind == "observe":
            return
        if kind in POSE_KINDS:
            if kind == "pose_skinned" and (self.skin is None or len(op["moves"]) <= self.max_bone()):
                return                                          # (only a replay with a bind left out comes here)
            p = self.stated(op)
            p.update(rebuilt=bool(op["rebuilt"]), kind=kind, moved=kind in ("pose_moved", "pose_skinned"))
            self.pose[op["dev"]] = p
        elif kind == "skin":
            self.skin = None if op["bones"] is None else dict(bones=op["bones"], weights=op["weights"], sphere_bone=op["sphere_bone"])
        elif kind == "resample":
            self.table = op["table"]
        elif kind == "reseed":
            self.table = ("seed", op["seed"], op["n_pairs"])
        else:
            raise KeyError(kind)

    def prims(self, posed, dev=0):
        if not posed:
            return self.created
        p = self.pose[dev]
        return {k: p[k] for k in ("tris", "spheres", "rgb", "sphere_rgb")}


# ------------------------------------------------------------------------------------------------ the draws
def rotation(rng, max_degrees=60.0):
    axis = rng.normal(size=3)
    axis /= np.linalg.norm(axis)
    a = np.deg2rad(rng.uniform(-max_degrees, max_degrees))
    k = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + np.sin(a) * k + (1 - np.cos(a)) * (k @ k)


def drawn_move(rng, sc):
    """a rotation about the scene's centre times a uniform scale in [0.5, 1.1], a small translation, sometimes a shear"""
    lin = rotation(rng) * rng.uniform(0.5, 1.1)
    if rng.random() < 0.25:
        sh = np.eye(3)
        sh[0, 1] = rng.uniform(-0.3, 0.3)
        lin = lin @ sh
    m = mv.about(lin, sc["centre"])
    m[[3, 7, 11]] = (m[[3, 7, 11]] + (rng.uniform(-0.05, 0.05, 3) * sc["scale"]).astype(F)).astype(F)
    return m


def drawn_colours(rng, n):
    c = rng.uniform(0.0, 1.0, size=(n, 3)).astype(F)
    if rng.random() < 0.3:
        c[:] = c[:, :1]
    return c


class Draw:
    """the seeded draw of one sequence; the log is self.log"""

    def __init__(self, sc, table, seed, steps, n_devices=1, index=0):
        self.sc, self.rng, self.steps, self.n_devices, self.index = sc, np.random.default_rng(seed), steps, n_devices, index
        self.seed = seed
        self.model = Model(sc, table, n_devices)
        self.log, self.pending, self.refusals = [], [], 0
        self.last_pose_kind = [None] * n_devices
        self.views = self.drawn_views()
        self.lights = [tuple(float(x) for x in self.drawn_light()) for _ in range(2)]
        n = len(sc["tris"])
        self.mesh = np.array([k for k in range(n) if k != sc["floor"]], np.int64)       # triangle numbers but the floor's

    # -- the pools
    def drawn_views(self):
        sc, rng = self.sc, self.rng
        views = [((sc["W"], sc["H"]), tuple(sc["kw"]["eye"]), tuple(sc["kw"]["look_at"]), float(sc["kw"]["distance"]))]
        bound = Model(sc, np.zeros((1, 2), F)).bound
        while len(views) < 3:
            d = rng.normal(size=3)
            eye = (sc["centre"] + d / np.linalg.norm(d) * sc["scale"] * rng.uniform(1.5, 3.5)).astype(F)
            if np.abs(eye).max() > bound:                       # the eye's range rule (rtx_render_view_rows)
                continue
            w, h = int(rng.integers(9, 33)), int(rng.integers(9, 25))
            views.append(((w, h), tuple(float(x) for x in eye), tuple(sc["kw"]["look_at"]), float(rng.uniform(0.6, 2.5) * max(w, h))))
        return views

    def drawn_light(self):
        sc, rng = self.sc, self.rng
        c = sc["centre"] + np.array([rng.uniform(-2, 2), rng.uniform(1.5, 4.0), rng.uniform(-2, 2)]) * sc["scale"]
        return (c + rng.uniform(-0.2, 0.2, size=(3, 3)) * sc["scale"]).astype(F).reshape(9)

    def device(self):
        return int(self.rng.integers(0, self.n_devices))

    # -- poses
    def moved_arrays(self):
        """the created triangles and spheres under one drawn move (the floor stays), by the numpy restatement"""
        sc = self.sc
        group = np.zeros(len(sc["kinds"]), np.uint32)
        if sc["floor"] is not None:
            group[self.model.tri_at[sc["floor"]]] = NONE
        return mv.restated(sc["tris"], sc["spheres"], sc["kinds"], drawn_move(self.rng, sc).reshape(1, 12), group, None)

    def draw_pose(self, kind, dev=None, variant=None, rebuilt=None, colours=None):
        sc, rng, m = self.sc, self.rng, self.model
        n_tris, n_sph, n_prims = len(sc["tris"]), len(sc["spheres"]), len(sc["kinds"])
        variant = variant or ("device" if rng.random() < 0.4 else "host")
        dev = 0 if variant == "device" else (self.device() if dev is None else dev)
        op = dict(op=kind, dev=dev, variant=variant, rgb=None, sphere_rgb=None,
                  rebuilt=(kind == "pose_rebuilt") if kind in ("pose", "pose_rebuilt") else bool(rng.integers(0, 2) if rebuilt is None else rebuilt))
        if colours is None:
            colours = rng.random() < 0.5
        if kind in ("pose", "pose_rebuilt"):
            op["tris"] = self.moved_arrays()[0]
        elif kind == "pose_prims":
            tris, spheres = self.moved_arrays()
            op["tris"] = tris
            op["spheres"] = spheres if n_sph and rng.random() < 0.5 else None
            op["rgb"] = drawn_colours(rng, n_tris) if n_tris and colours else None
            op["sphere_rgb"] = drawn_colours(rng, n_sph) if n_sph and (colours if not n_tris else rng.random() < 0.5) else None
        elif kind == "pose_moved":
            n_moves = int(rng.integers(1, 9))
            op["moves"] = np.stack([drawn_move(rng, sc) for _ in range(n_moves)]).astype(F)
            if rng.random() < 0.2:
                op["group"] = None
            else:
                g = rng.integers(0, n_moves, n_prims).astype(np.uint32)
                g[rng.random(n_prims) < 0.2] = NONE
                if variant == "device":                         # whatever a device array holds: taken as RTX_MOVE_NONE
                    wild = rng.random(n_prims) < 0.1
                    g[wild] = np.array([n_moves, n_moves + 1, 0xFFFFFFFE], np.uint32)[rng.integers(0, 3, int(wild.sum()))]
                if sc["floor"] is not None:
                    g[m.tri_at[sc["floor"]]] = NONE
                op["group"] = g
            op["radius_scale"] = rng.uniform(0.5, 1.2, n_moves).astype(F) if rng.random() < 0.5 else None
            op["rgb"] = drawn_colours(rng, n_tris) if n_tris and colours else None
            op["sphere_rgb"] = drawn_colours(rng, n_sph) if n_sph and colours else None
        elif kind == "pose_skinned":
            if m.skin is None:
                return None
            n_moves = m.max_bone() + 1 + int(rng.integers(0, 3))
            op["moves"] = np.stack([drawn_move(rng, sc) for _ in range(n_moves)]).astype(F)
            op["radius_scale"] = rng.uniform(0.5, 1.2, n_moves).astype(F) if rng.random() < 0.5 else None
            op["rgb"] = drawn_colours(rng, n_tris) if n_tris and colours else None
            op["sphere_rgb"] = drawn_colours(rng, n_sph) if n_sph and colours else None
        # the blocking read-back of what the device holds: always after a host variant, after a device variant by a draw
        op["read_back"] = bool(variant == "host" or rng.random() < 0.5)
        p = m.stated(op)
        return op if m.in_range(p["tris"], p["spheres"]) else None

    def draw_skin(self, n_bones=None):
        sc, rng = self.sc, self.rng
        n_tris, n_sph = len(sc["tris"]), len(sc["spheres"])
        n_bones = int(rng.choice([2, 3, 5, 8])) if n_bones is None else n_bones
        s = sk.dealt_skin(n_tris, n_sph, n_bones, int(rng.integers(0, 2 ** 31)))
        shift = int(rng.integers(0, n_bones))                   # (another deal per bind)
        b = s["bones"]
        s["bones"] = np.where(b == NONE, b, (b + np.uint32(shift)) % np.uint32(n_bones)).astype(np.uint32)
        if sc["floor"] is not None:
            s["bones"][sc["floor"]] = NONE
        if n_tris:                                              # the largest bone is n_bones - 1 whatever the deal
            t = int(self.mesh[0])
            s["bones"][t, 0, 0] = n_bones - 1
        elif n_sph:
            s["sphere_bone"][0] = n_bones - 1
        return dict(op="skin", bones=s["bones"], weights=s["weights"], sphere_bone=s["sphere_bone"])

    def draw_table(self):
        rng = self.rng
        if rng.random() < 0.5:
            n = int(rng.choice(TABLE_PAIRS))
            return dict(op="resample", table=rng.uniform(0.0, 1.0, size=(n, 2)).astype(F), read_back=bool(rng.integers(0, 2)))
        return dict(op="reseed", seed=int(rs.SEEDS[int(rng.integers(0, len(rs.SEEDS)))]), n_pairs=int(rng.choice(SEED_PAIRS)),
                    read_back=bool(rng.integers(0, 2)))

    # -- refused calls: every one decided on the host, before a device is looked for
    def draw_refusal(self, only=None):
        sc, rng, m = self.sc, self.rng, self.model
        n_prims = len(sc["kinds"])
        for k in range(len(REFUSALS)):
            name = REFUSALS[(self.refusals + self.index + k) % len(REFUSALS)]
            if only is not None and name != only:
                continue
            dev = self.device()
            moves = np.stack([drawn_move(rng, sc) for _ in range(2)]).astype(F)
            op = None
            if name == "skinned_without_skin" and m.skin is None:
                op = dict(op="pose_skinned", moves=moves, radius_scale=None, group=None, code=ERR_BAD_ARG)
            elif name == "skinned_with_group" and m.skin is not None:
                n = m.max_bone() + 1
                op = dict(op="pose_skinned", moves=np.stack([drawn_move(rng, sc) for _ in range(n)]).astype(F), radius_scale=None,
                          group=np.full(n_prims, NONE, np.uint32), code=ERR_BAD_ARG)
            elif name == "skinned_few_moves" and m.skin is not None and m.max_bone() >= 1:
                n = m.max_bone()
                op = dict(op="pose_skinned", moves=np.stack([drawn_move(rng, sc) for _ in range(n)]).astype(F), radius_scale=None,
                          group=None, code=ERR_BAD_ARG)
            elif name == "moved_out_of_bound":
                far = mv.about(np.eye(3) * 8.0, sc["centre"] + sc["scale"]).reshape(1, 12)
                t, s = mv.restated(sc["tris"], sc["spheres"], sc["kinds"], far, None, None)
                if not m.in_range(t, s):
                    op = dict(op="pose_moved", moves=far, group=None, radius_scale=None, code=ERR_UNSUPPORTED)
            elif name == "posed_without_pose":
                free = [d for d in range(self.n_devices) if m.pose[d] is None]
                if free:
                    op = self.draw_observation(posed=True, dev=free[0], kind="render_view", force=True)
                    op.update(code=ERR_BAD_ARG)
            elif name == "bad_group":
                g = rng.integers(0, 2, n_prims).astype(np.uint32)
                g[int(rng.integers(0, n_prims))] = 2 + int(rng.integers(0, 2)) * 0xFFFFFFFC
                op = dict(op="pose_moved", moves=moves, group=g, radius_scale=None, code=ERR_BAD_ARG)
            elif name == "resample_nothing":
                op = dict(op="resample", table=np.zeros((0, 2), F), code=ERR_BAD_ARG)
            if op is not None:
                self.refusals += 1
                op.setdefault("dev", dev)
                op.update(refused=name, variant="host", rebuilt=bool(rng.integers(0, 2)), rgb=None, sphere_rgb=None)
                return op
        return None

    # -- observations
    def view_rays(self, v):
        (w, h), eye, look_at, distance = self.views[v]
        o, d = ray_arrays(w, h, eye, look_at, distance, self.model.table_array(), self.sc["kw"]["nb_ray"])
        return o, d

    def draw_observation(self, posed=None, dev=None, kind=None, view=None, light="draw", force=False, window=None, whole=False):
        """whole: the whole frame or the largest batch — what follows a state change, so that the change is seen"""
        sc, rng, m = self.sc, self.rng, self.model
        for _ in range(REDRAWS + 1):
            ob = dict(op="observe")
            ob["dev"] = self.device() if dev is None else dev
            can_pose = m.pose[ob["dev"]] is not None
            ob["posed"] = (bool(rng.random() < 0.65) and can_pose) if posed is None else posed
            if ob["posed"] and not can_pose and not force:
                ob["posed"] = False
            kinds = ["render_rows", "render_frame", "render_view", "render_view_rows", "render_view_rows", "shade_rays", "trace_rays",
                     "occluded_rays", "render_view_rows_device", "render_view_device", "shade_rays_device"]
            if ob["posed"]:
                kinds = kinds[2:]
            ob["kind"] = kinds[int(rng.integers(0, len(kinds)))] if kind is None else kind
            if ob["kind"].endswith("_device") or ob["kind"] == "render_frame":
                ob["dev"] = 0
                if ob["posed"] and m.pose[0] is None:
                    continue
            k = ob["kind"]
            own = k in ("render_rows", "render_frame")
            if own:                                             # the scene's own frame has no posed form
                ob["posed"] = False
            ob["view"] = 0 if own else (int(rng.integers(0, 3)) if view is None else view)
            (w, h) = self.views[ob["view"]][0]
            ob["light"] = None
            if not own and k not in ("trace_rays", "occluded_rays"):
                if light == "draw":
                    if rng.random() < 0.45:
                        tri = None if rng.random() < 0.3 else self.lights[int(rng.integers(0, 2))]
                        ob["light"] = (tri if tri is not None else tuple(sc["kw"]["light_tri"]), int(rng.choice(LIGHT_COUNTS)))
                else:
                    ob["light"] = light
            if k in ("render_rows", "render_view_rows", "render_view_rows_device"):
                if window is not None:
                    ob["window"] = window
                else:
                    y0 = int(rng.integers(0, h))
                    ob["window"] = (0, h) if whole or rng.random() < 0.3 else (y0, int(rng.integers(1, h - y0 + 1)))
            elif k in ("render_view", "render_view_device"):
                x0, y0 = int(rng.integers(0, w)), int(rng.integers(0, h))
                ob["rect"] = (0, 0, w, h) if whole or rng.random() < 0.3 else (x0, y0, int(rng.integers(1, w - x0 + 1)), int(rng.integers(1, h - y0 + 1)))
                ob["want_shade"], ob["want_hits"] = bool(rng.integers(0, 2)), bool(rng.integers(0, 2)) and k == "render_view"
            elif k in ("shade_rays", "trace_rays", "occluded_rays", "shade_rays_device"):
                nb = sc["kw"]["nb_ray"]
                o, d = self.view_rays(ob["view"])
                n = BATCHES[-1] if whole else int(rng.choice(BATCHES))
                if k.startswith("shade"):                       # whole pixels: nb_ray consecutive rays each
                    count = ob["light"][1] if ob["light"] is not None and ob["light"][1] else sc["kw"]["nb_light_sample"]
                    if count >= 100:
                        n = min(n, 65)                          # (the composition is a Python loop per shadow ray)
                    n_px = min(max(n // nb, 1), w * h)
                    p0 = int(rng.integers(0, w * h - n_px + 1))
                    sel = slice(p0 * nb, (p0 + n_px) * nb)
                else:
                    n = min(n, len(o))
                    r0 = int(rng.integers(0, len(o) - n + 1))
                    sel = slice(r0, r0 + n)
                ob["origins"], ob["second"] = np.ascontiguousarray(o[sel]), np.ascontiguousarray(d[sel])
                ob["order"] = ("keep_order", "force_regroup", "none")[int(rng.integers(0, 3))]
                ob["want_hits"] = bool(rng.integers(0, 2)) and k == "shade_rays"
                if k == "occluded_rays":                        # targets around the scene: the ray scaled to the eye's distance
                    reach = np.linalg.norm(np.asarray(self.views[ob["view"]][1]) - sc["centre"]) / self.views[ob["view"]][3]
                    f = (reach * rng.uniform(0.3, 1.6, size=(len(ob["origins"]), 1))).astype(F)
                    ob["second"] = (ob["origins"] + (ob["second"] * f).astype(F)).astype(F)
                    if not ((ob["second"] - ob["origins"]).astype(F) != 0).all():
                        continue
            if True:                                            # no ray direction may have a zero component
                o, d = self.view_rays(ob["view"])
                if not (d != 0).all():
                    continue
            return ob
        raise RuntimeError("no observation inside the contract after %d draws" % (REDRAWS + 1))

    # -- the sequence
    def follow(self, op):
        """what a state change or an observation asks the next steps to be"""
        rng, m = self.rng, self.model
        kind = op["op"]
        if kind in POSE_KINDS:
            r = rng.random()
            if r < 0.25:                                        # a table change between the pose and its observation
                self.pending.append(lambda: self.draw_table())
            if r < 0.9:
                dev = op["dev"]
                host = op["variant"] == "device" and rng.random() < 0.6
                frames = ("render_view_rows", "render_view") if host or dev else ("render_view_rows", "render_view", "render_view_rows_device",
                                                                                  "render_view_device")
                others = ("shade_rays", "trace_rays", "occluded_rays") if host or dev else ("shade_rays", "trace_rays", "occluded_rays",
                                                                                          "shade_rays_device")
                pick = frames if rng.random() < 0.9 else others
                self.pending.append(lambda: self.draw_observation(posed=True, dev=dev, kind=pick[int(rng.integers(0, len(pick)))], whole=True))
        elif kind in ("resample", "reseed"):
            if rng.random() < 0.9:
                kinds = ("render_rows", "render_frame", "render_view", "render_view_rows", "shade_rays", "render_view_rows_device")
                self.pending.append(lambda: self.draw_observation(kind=kinds[int(rng.integers(0, len(kinds)))], whole=True))
        elif kind == "skin" and op["bones"] is not None:
            if rng.random() < 0.9:
                self.pending.append(lambda: self.draw_pose("pose_skinned"))
        elif kind == "observe" and not op.get("twin"):
            r = rng.random()
            k = op["kind"]
            if k.startswith("render_view_rows") and op["posed"] and r < 0.5:
                if r < 0.25:                                    # an unposed window of the same eye
                    twin = dict(posed=False, view=op["view"])
                else:                                           # a posed one of another eye
                    twin = dict(posed=True, view=(op["view"] + 1 + int(rng.integers(0, 2))) % 3)
                self.pending.insert(0, lambda: dict(self.draw_observation(dev=op["dev"], kind=k, light=op["light"], **twin), twin=True))
            elif "light" in op and k not in ("render_rows", "render_frame", "trace_rays", "occluded_rays") and r < 0.35:
                other = None if op["light"] is not None else (self.lights[int(rng.integers(0, 2))], int(rng.choice(LIGHT_COUNTS)))
                self.pending.insert(0, lambda: dict({a: b for a, b in op.items() if a != "light"}, light=other, twin=True))

    def step(self):
        rng, m = self.rng, self.model
        if self.pending:
            op = self.pending.pop(0)()
            if op is not None:
                return op
        r = rng.random()
        for _ in range(REDRAWS):
            op = None
            if r < 0.36:
                weights = np.array([1.0, 1.0, 1.3, 1.5, 1.7 if m.skin is not None else 0.0])
                if not len(self.sc["tris"]):                    # no triangle to state: the kinds that state more
                    weights[:2] = 0.0
                kind = POSE_KINDS[int(rng.choice(5, p=weights / weights.sum()))]
                last, colours = self.last_pose, None
                if last is not None and coloured(last):
                    colours = bool(rng.random() < 0.25)         # a pose with colours, then mostly one without
                op = self.draw_pose(kind, colours=colours)
            elif r < 0.44:
                op = self.draw_table()
            elif r < 0.53:
                if m.skin is not None and rng.random() < 0.25:
                    op = dict(op="skin", bones=None, weights=None, sphere_bone=None)
                elif m.skin is not None and rng.random() < 0.5:  # a re-bind to a smaller largest bone
                    smaller = [n for n in (2, 3, 5) if n - 1 < m.max_bone()]
                    op = self.draw_skin(n_bones=int(rng.choice(smaller)) if smaller else None)
                else:
                    op = self.draw_skin()
            elif r < 0.62:
                op = self.draw_refusal()
            else:
                op = self.draw_observation()
            if op is not None:
                return op
        return self.draw_observation()

    @property
    def last_pose(self):
        poses = [o for o in self.log if o["op"] in POSE_KINDS and not o.get("refused")]
        return poses[-1] if poses else None

    def scripted(self):
        """the first steps of a sequence: a posed call on a device without a pose, a bind, and a chain of pose kinds dealt by
        the sequence's index so that the twelve sequences together hold every ordered pair"""
        first = self.draw_observation(posed=True, dev=0, kind="render_view_rows", force=True, light=None)
        first.update(code=ERR_BAD_ARG, refused="posed_without_pose", variant="host")
        out = [lambda: first, lambda: self.draw_refusal(only="skinned_without_skin"), lambda: self.draw_skin()]
        pairs = [(a, b) for a in range(5) for b in range(5)]
        mine = pairs[self.index % 12::12]                       # two or three pairs each
        for a, b in mine:
            for k in (a, b):
                if not len(self.sc["tris"]) and k < 2:
                    k += 2
                out.append(lambda k=k: self.draw_pose(POSE_KINDS[k], dev=0))
                out.append(lambda: self.draw_observation(posed=self.model.pose[0] is not None, dev=0, whole=True))
        return out

    def run(self):
        self.pending = self.scripted()
        while len(self.log) < self.steps:
            op = self.step()
            op["step"] = len(self.log)
            self.model.apply(op)
            self.log.append(op)
            if not op.get("refused"):
                self.follow(op)
        return self.log


def ray_arrays(w, h, eye, look_at, distance, table, nb_ray):
    """shade_sets.camera_raw_rays without the oracle: Camera::new and create_rays in f32 (np_ref has both)"""
    u, v, wv = np_ref.camera_new(eye, look_at, UP)
    py, px = np.divmod(np.arange(w * h, dtype=np.uint32), np.uint32(w))
    d = np.zeros((w * h, nb_ray, 3), F)
    for i in range(nb_ray):
        k = (px * np.uint32(w) + py + np.uint32(i)) % np.uint32(len(table))
        a = px.astype(F) - F(w) / F(2.0) + table[k, 0]
        b = py.astype(F) - F(h) / F(2.0) + table[k, 1]
        for c in range(3):
            d[:, i, c] = (a * u[c] + b * v[c]) - F(distance) * wv[c]
    o = np.broadcast_to(np.asarray(eye, F), (w * h * nb_ray, 3)).copy()
    return o, d.reshape(-1, 3)


def sequence_seed(index):
    return int(os.environ.get("RTX_SEQUENCE_SEED", BASE_SEED + index))


def sequence_steps():
    return int(os.environ.get("RTX_SEQUENCE_STEPS", STEPS))


def draw_log(index, table, n_devices=1, seed=None, steps=None):
    """-> (scene dict, Draw) of family member `index`: the log is Draw.log"""
    sc = family_scene(FAMILY[index])
    d = Draw(sc, table, sequence_seed(index) if seed is None else seed, sequence_steps() if steps is None else steps, n_devices, index)
    d.run()
    return sc, d


def describe(op):
    """one line of the operation log"""
    def short(v):
        if isinstance(v, np.ndarray):
            return "%s%s#%s" % (v.dtype.char, list(v.shape), digest(v)[:6])
        if isinstance(v, tuple) and len(v) == 2 and isinstance(v[0], tuple):      # a light: its triangle and count
            return "(tri#%s, %d)" % (digest(np.asarray(v[0], F))[:6], v[1])
        return repr(v)
    return "%3d %s" % (op["step"], " ".join("%s=%s" % (k, short(v)) for k, v in op.items() if k != "step" and v is not None))


def log_text(log, upto=None):
    return "\n".join(describe(op) for op in log[:None if upto is None else upto + 1])


# ------------------------------------------------------------------------------------------------ the oracle's answers
THREADS = 8


class Expect:
    """the oracle's answer for an observation on a model: a fresh oracle scene per (primitives, table, light, camera),
    results cached by that state"""

    def __init__(self, orc, sc, views):
        self.orc, self.sc, self.views = orc, sc, views
        self.frames, self.windows, self.scenes, self.prim_tables, self.rays = {}, {}, {}, {}, {}

    def close(self):
        for osc in self.scenes.values():
            osc.close()
        self.scenes = {}

    def light_of(self, light):
        kw = self.sc["kw"]
        if light is None:
            return tuple(kw["light_tri"]), kw["nb_light_sample"]
        return tuple(light[0]), (light[1] or kw["nb_light_sample"])

    def oracle_scene(self, prims, table, light, v):
        sc = self.sc
        (w, h), eye, look_at, distance = self.views[v]
        tri, count = self.light_of(light)
        extra = dict(spheres=prims["spheres"], sphere_rgb=prims["sphere_rgb"], kinds=sc["kinds"]) if len(sc["spheres"]) else {}
        return self.orc.Scene(w, h, prims["tris"], prims["rgb"], table, eye=eye, look_at=look_at, up=UP, distance=distance,
                              light_tri=tri, nb_ray=sc["kw"]["nb_ray"], nb_light_sample=count, **extra)

    def state_key(self, model, ob):
        prims = model.prims(ob["posed"], ob["dev"])
        return (digest(prims["tris"], prims["spheres"], prims["rgb"], prims["sphere_rgb"]), model.table_key(),
                self.light_of(ob.get("light")), ob["view"])

    def frame(self, model, ob):
        """the whole frame of the observation's view -> dict(frame, stats, tri, lin)"""
        key = self.state_key(model, ob)
        if key not in self.frames:
            osc = self.oracle_scene(model.prims(ob["posed"], ob["dev"]), model.table_array(), ob.get("light"), ob["view"])
            frame, st, tri, lin = osc.render_rows(mode=self.orc.MODE_BVH, nthreads=THREADS, want_tri=True, want_lin=True)
            osc.close()
            self.frames[key] = dict(frame=frame, stats=st, tri=tri, lin=lin)
        return self.frames[key]

    def window_hits(self, model, ob, rect):
        """primary hits of the rectangle alone, by the oracle's own window render"""
        key = self.state_key(model, ob) + (rect,)
        if key not in self.windows:
            osc = self.oracle_scene(model.prims(ob["posed"], ob["dev"]), model.table_array(), ob.get("light"), ob["view"])
            _, st = osc.render_window(*rect, mode=self.orc.MODE_BVH, nthreads=THREADS)
            osc.close()
            self.windows[key] = st["primary_hits"]
        return self.windows[key]

    def geometry(self, prims):
        """an oracle scene holding the primitives (closest hits depend on nothing else) and shade_sets.prim_tables of them"""
        key = digest(prims["tris"], prims["spheres"], prims["rgb"], prims["sphere_rgb"])
        if key not in self.scenes:
            self.scenes[key] = self.oracle_scene(prims, np.zeros((1, 2), F), None, 0)
            self.prim_tables[key] = ss.prim_tables(self.orc, prims["tris"], prims["rgb"], prims["spheres"], prims["sphere_rgb"], self.sc["kinds"])
        return self.scenes[key], self.prim_tables[key]

    def observation(self, model, ob):
        """-> dict(skip: the oracle reports a non-finite hit distance in the view, bytes: everything compared, as one
        string, and the parts by name)"""
        orc, k = self.orc, ob["kind"]
        fr = self.frame(model, ob)
        out = dict(skip=bool(fr["stats"]["nonfinite_t"]))
        (w, h) = self.views[ob["view"]][0]
        if k in ("render_rows", "render_view_rows", "render_view_rows_device"):
            y0, ny = ob["window"]
            out.update(rgb=fr["frame"][y0:y0 + ny], primary_hits=self.window_hits(model, ob, (0, y0, w, ny)))
        elif k == "render_frame":
            out.update(rgb=fr["frame"], primary_hits=fr["stats"]["primary_hits"])
        elif k in ("render_view", "render_view_device"):
            x0, y0, nx, ny = ob["rect"]
            ys, xs = slice(y0, y0 + ny), slice(x0, x0 + nx)
            out.update(rgb=fr["frame"][ys, xs], lin=fr["lin"][ys, xs], tri=fr["tri"][ys, xs], primary_hits=self.window_hits(model, ob, ob["rect"]))
        else:
            prims = model.prims(ob["posed"], ob["dev"])
            key = (digest(prims["tris"], prims["spheres"], prims["rgb"], prims["sphere_rgb"]), digest(ob["origins"], ob["second"]), k,
                   model.table_key() if k.startswith("shade") else None, self.light_of(ob.get("light")) if k.startswith("shade") else None)
            if key not in self.rays:
                osc, tables = self.geometry(prims)
                if k == "trace_rays":
                    exp, _ = qs.oracle_hits(orc, osc, ob["origins"], ob["second"], qs.HIT_DTYPE)
                    self.rays[key] = dict(hits=exp, tables=tables)
                elif k == "occluded_rays":
                    exp, _ = qs.oracle_hits(orc, osc, ob["origins"], (ob["second"] - ob["origins"]).astype(F), qs.HIT_DTYPE)
                    self.rays[key] = dict(occluded=qs.expected_occlusion(exp, ob["origins"], ob["second"]))
                else:
                    tri, count = self.light_of(ob.get("light"))
                    s = ss.shade_set(orc, osc, ob["origins"], ob["second"], self.sc["kw"]["nb_ray"], count, tri, model.table_array(), tables)
                    self.rays[key] = dict(shade=s["shade"], hits=s["hit"], tables=tables)
            out.update(self.rays[key])
        out["bytes"] = b"".join(np.ascontiguousarray(out[n]).tobytes() for n in ("rgb", "lin", "tri", "hits", "occluded", "shade") if n in out)
        return out


# ------------------------------------------------------------------------------------------------ what a log holds
def coloured(op):
    return op.get("rgb") is not None or op.get("sphere_rgb") is not None


def is_twin(a, b, ignore):
    keys = (set(a) | set(b)) - {"step", "twin"} - set(ignore)
    same = lambda x, y: (np.array_equal(x, y) if isinstance(x, np.ndarray) or isinstance(y, np.ndarray) else x == y)
    return all(k in a and k in b and same(a[k], b[k]) for k in keys)


def coverage(log):
    """the transitions of the coverage table that this log holds -> dict of sets / booleans (test_sequence_model joins the
    twelve)"""
    ok = [op for op in log if not op.get("refused")]
    c = dict(pairs=set(), kinds_rebuilt=set(), rebuilt_then_refitted=False, refitted_then_rebuilt=False, colours_then_none=False,
             table_between_pose_and_posed=False, rebind_between_skinned=False, rebind_to_smaller=False, unbind=False,
             lit_then_unlit=False, unlit_then_lit=False, posed_window_then_unposed_same_eye=False, posed_window_then_posed_other_eye=False,
             device_pose_then_host_observation=False, refusals={op["refused"] for op in log if op.get("refused")})
    last_pose, table_since, skin_state, bone = {}, {}, None, None
    for prev, op in zip([None] + ok[:-1], ok):
        kind = op["op"]
        if kind in POSE_KINDS:
            before = last_pose.get(op["dev"])
            c["kinds_rebuilt"].add((kind, bool(op["rebuilt"])))
            if before is not None:
                c["pairs"].add((before["op"], kind))
                c["rebuilt_then_refitted"] |= bool(before["rebuilt"] and not op["rebuilt"])
                c["refitted_then_rebuilt"] |= bool(not before["rebuilt"] and op["rebuilt"])
                c["colours_then_none"] |= before["op"] in ("pose_prims", "pose_moved") and coloured(before) and not coloured(op)
            last_pose[op["dev"]] = op
            table_since[op["dev"]] = False
            if kind == "pose_skinned":
                if skin_state == "rebound":
                    c["rebind_between_skinned"] = True
                    c["rebind_to_smaller"] |= bool(bone[1] < bone[0])
                skin_state = "posed"
        elif kind in ("resample", "reseed"):
            table_since = {d: True for d in table_since}
        elif kind == "skin":
            if op["bones"] is None:
                c["unbind"], skin_state = True, None
            else:
                b = np.concatenate([op["bones"].reshape(-1), op["sphere_bone"].reshape(-1)])
                top = int(b[b != NONE].max())
                if skin_state == "posed":
                    skin_state, bone = "rebound", (bone_now, top)
                elif skin_state == "rebound":
                    bone = (bone[0], top)
                bone_now = top
        else:
            if op["posed"] and table_since.get(op["dev"]):
                c["table_between_pose_and_posed"] = True
            if op["posed"]:
                table_since[op["dev"]] = False
            if prev is not None and prev["op"] == "observe":
                if "light" in op and is_twin(prev, op, ("light",)):
                    c["lit_then_unlit"] |= prev["light"] is not None and op["light"] is None
                    c["unlit_then_lit"] |= prev["light"] is None and op["light"] is not None
                if prev["kind"].startswith("render_view_rows") and op["kind"].startswith("render_view_rows") and prev["posed"]:
                    c["posed_window_then_unposed_same_eye"] |= not op["posed"] and op["view"] == prev["view"]
                    c["posed_window_then_posed_other_eye"] |= op["posed"] and op["view"] != prev["view"]
            if prev is not None and prev["op"] in POSE_KINDS and prev["variant"] == "device":
                c["device_pose_then_host_observation"] |= op["posed"] and op["dev"] == 0 and not op["kind"].endswith("_device")
    return c


def state_changes(log):
    """steps of the log that change what a later observation may return"""
    return [op["step"] for op in log if not op.get("refused") and op["op"] != "observe"
            and not (op["op"] == "skin" and op["bones"] is None)]
