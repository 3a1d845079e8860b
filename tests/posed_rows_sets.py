"""Fixtures for the tests of rtx_render_view_rows_posed (a pose through the render pipeline), with the CPU oracle's answers:
numpy, the oracle binding and the library's host side only, no GPU.  pose_sets (the five bunny poses at the 44 x 27 "side"
view, the small scenes, POSE_LIGHT, the 24 x 16 turntable) and lit_rows_sets serve as they are; what is added here:

LIFTED GROUND, the scene a stale plane record gets wrong.  A ground triangle as large as the scene at y = 0 (the scene's one
global triangle), a patch of small triangles a little above it, the light above the patch, and a camera that looks down on
the patch from above and from the side.  The pose lifts ONLY the ground, to a height between the patch and the light.  The
ground's edge x = 4 runs beside the patch: the patch lies under the lifted ground, the camera looks in past the edge.  So
under the pose the primary rays left of the edge meet the lifted ground first, the others still find the patch, and every
shadow ray of the patch is occluded by the ground above it.  A library that kept the plane record of the ground at y = 0
would certify exactly those shadow rays as "moving away" from it (origin above the plane, direction upwards), leave the
ground out of their walks, and light the patch.

Also here: a numpy restatement of the certificate (rtx_traverse.hpp: plane_origin / plane_rules_out) that reports by how
much a ray clears the inequality it is certified by, a pure-Python restatement of the plane statement (scene_prep.h:
global_plane_statement; Python floats are doubles), and the list of (scene, pose, eyes) the record comparisons run over.
tests/test_posed_rows_sets.py asserts, without a GPU, the conditions these fixtures must meet;
tests/test_gpu_posed_rows.py uses them.  Everything is built once per process (query_sets._once)."""
import struct

import numpy as np

import pose_sets as ps
import query_sets as qs
import shade_sets as ss
import view_sets as vs
from query_sets import F, NO_HIT

# ---- the lifted ground -------------------------------------------------------------------------------------------------
LIFT_GROUND = np.array([4.0, 0.0, -100.0, 4.0, 0.0, 100.0, -196.0, 0.0, 0.0], F)
LIFT_HEIGHT = 7.0
LIFT_LIGHT = (-1.0, 12.0, -1.0, 1.0, 12.0, -1.0, 0.0, 12.0, 1.0)
LIFT_NB_LIGHT = 6
LIFT_VIEW = ((16, 14), (60.0, 40.0, 9.0), (0.0, 2.0, 0.0), 95.0)
LIFT_BOUND = 196.0                        # the largest coordinate magnitude of the created scene and its eye: the pose bound


def lift_tris():
    """the patch — a 3 x 3 grid of quads, 18 triangles over [-3, 3]^2 whose height waves between 2 and 2.6 — then the ground"""
    g = np.linspace(-3.0, 3.0, 4)
    h = lambda x, z: 2.3 + 0.3 * np.sin(1.3 * x + 0.7 * z)
    out = []
    for i in range(3):
        for k in range(3):
            x0, x1, z0, z1 = g[i], g[i + 1], g[k], g[k + 1]
            a, b, c, d = (x0, h(x0, z0), z0), (x1, h(x1, z0), z0), (x1, h(x1, z1), z1), (x0, h(x0, z1), z1)
            out += [a + b + c, a + c + d]
    return np.ascontiguousarray(np.concatenate([np.array(out, F), LIFT_GROUND.reshape(1, 9)]))


def lift_rgb():
    n = len(lift_tris())
    rgb = np.tile(np.array([0.9, 0.8, 0.3], F), (n, 1))
    rgb[-1] = (0.4, 0.6, 0.9)
    return np.ascontiguousarray(rgb)


def lift_pose():
    pose = lift_tris().copy()
    pose[-1, 1::3] = F(LIFT_HEIGHT)
    return np.ascontiguousarray(pose)


LIFT_GROUND_INDEX = 18


def lift_kw():
    return dict(vs.camera(LIFT_VIEW), light_tri=LIFT_LIGHT, nb_ray=1, nb_light_sample=LIFT_NB_LIGHT)


def lift_scene(rtx, samples, **more):
    """the library's scene, created with the UNPOSED triangles and LIFT_VIEW's frame and camera"""
    return rtx.Scene(LIFT_VIEW[0][0], LIFT_VIEW[0][1], lift_tris(), lift_rgb(), samples, **dict(lift_kw(), **more))


def lifted(orc, samples):
    """dict(frame / stats / tri = the oracle scene created with the POSED vertices, still = the unposed oracle frame,
    rays = (origins, unit directions, is_shadow) of every ray of the posed frame whose oracle answer is the lifted ground:
    primary rays and the shadow rays of the primary hits)"""
    def make():
        (w, h) = LIFT_VIEW[0]
        osc = orc.Scene(w, h, lift_pose(), lift_rgb(), samples, **lift_kw())
        frame, st, tri = osc.render_rows(mode=orc.MODE_BVH, want_tri=True)
        plain = orc.Scene(w, h, lift_tris(), lift_rgb(), samples, **lift_kw())
        still = plain.render_rows(mode=orc.MODE_BVH)[0]
        plain.close()
        o, d, _, _, _ = ss.camera_raw_rays(orc, w, h, LIFT_VIEW[1], LIFT_VIEW[2], vs.UP, LIFT_VIEW[3], samples, 1)
        exp, units = qs.oracle_hits(orc, osc, o, d, qs.HIT_DTYPE)
        assert np.array_equal(exp["prim"].reshape(h, w), tri)
        lp = ss.light_points(orc, LIFT_LIGHT, samples, 1, LIFT_NB_LIGHT)[0]
        hit = np.nonzero(exp["prim"] != NO_HIT)[0]
        so = np.repeat(exp["p_hit"][hit], LIFT_NB_LIGHT, axis=0)
        sd = (np.tile(lp, (len(hit), 1)) - so).astype(F)
        sexp, sunits = qs.oracle_hits(orc, osc, so, sd, qs.HIT_DTYPE)
        from_patch = np.repeat(exp["prim"][hit] != LIFT_GROUND_INDEX, LIFT_NB_LIGHT)
        on_p, on_s = exp["prim"] == LIFT_GROUND_INDEX, sexp["prim"] == LIFT_GROUND_INDEX
        rays = (np.concatenate([o[on_p], so[on_s]]), np.concatenate([units[on_p], sunits[on_s]]),
                np.concatenate([np.zeros(int(on_p.sum()), bool), np.ones(int(on_s.sum()), bool)]))
        osc.close()
        for a in (frame, still, tri):
            a.setflags(write=False)
        return dict(frame=frame, stats=st, tri=tri, still=still, rays=rays, patch_pixels=int((tri < LIFT_GROUND_INDEX).sum()),
                    ground_pixels=int((tri == LIFT_GROUND_INDEX).sum()), patch_shadow_rays=int(from_patch.sum()),
                    patch_shadow_rays_on_ground=int((from_patch & on_s).sum()))
    return qs._once("posed_rows_lifted", make)


# ---- the certificate, restated (rtx_traverse.hpp: plane_origin, plane_rules_out) -----------------------------------------
K = F(2.0 ** -19)
TINY = F(2.0 ** -100)


def _fma(a, b, c):
    """one fused step: the f32 product formed in float64 (exact), the sum rounded once to f32"""
    return (np.asarray(a, F).astype(np.float64) * np.asarray(b, F).astype(np.float64) + np.asarray(c, F).astype(np.float64)).astype(F)


def certificate(plane, o, d):
    """plane: one 16-word record (v0, N, W, K_d, ...) as uint32 or float32; o, d: [n, 3] float32.
    -> (certified out [n], clearance [n]: the largest factor by which a certified ray clears an inequality it is certified
    by — rhs / lhs of "magnitude", and for "moving away" the smaller of |s_n| / kA_n and |s_d| / K_d —, 0 where not)"""
    g = np.asarray(plane).view(F).reshape(16)
    v0, n, w, kd = g[0:3], g[3:6], g[6:9], g[9]
    o, d = np.asarray(o, F), np.asarray(d, F)
    with np.errstate(all="ignore"):
        tv = (o - v0).astype(F)
        sn = _fma(tv[:, 2], n[2], _fma(tv[:, 1], n[1], tv[:, 0] * n[0]))
        an = _fma(np.abs(tv[:, 2]), w[2], _fma(np.abs(tv[:, 1]), w[1], np.abs(tv[:, 0]) * w[0]))
        kan = _fma(an, K, TINY)
        lhs = ((np.abs(sn) + kan) * (F(1.0) + K)).astype(F)
        sn_kept = np.where(np.abs(sn) > kan, sn, F(0.0)).astype(F)
        sd = _fma(d[:, 2], n[2], _fma(d[:, 1], n[1], d[:, 0] * n[0]))
        rhs = (np.abs(sd) - kd).astype(F)
        magnitude = lhs < rhs
        away = ((sn_kept * sd).astype(F) > 0) & (np.abs(sd) > kd)
        c_mag = np.where(magnitude, rhs.astype(np.float64) / np.maximum(lhs.astype(np.float64), 1e-300), 0.0)
        c_away = np.where(away, np.minimum(np.abs(sn).astype(np.float64) / np.maximum(float(1) * kan.astype(np.float64), 1e-300),
                                           np.abs(sd).astype(np.float64) / max(float(kd), 1e-300)), 0.0)
    return magnitude | away, np.maximum(c_mag, c_away)


# ---- the plane statement, restated in Python floats (doubles) -------------------------------------------------------------
def _f32(x):
    """a double rounded to the nearest f32 (overflow: infinity), as a double"""
    try:
        return struct.unpack("<f", struct.pack("<f", x))[0]
    except OverflowError:
        return float("inf") if x > 0 else float("-inf")


def _up(x):
    """the f32 above the f32 x >= +0: one more in the bit pattern; infinity and a NaN stay"""
    if not x < float("inf"):
        return x
    return struct.unpack("<f", struct.pack("<I", struct.unpack("<I", struct.pack("<f", x))[0] + 1))[0]


def plane_words(tri_words):
    """one primitive record (16 words: v0, e1, e2, own box, idx) -> its plane record's 16 words"""
    t = np.asarray(tri_words, np.uint32).reshape(16)
    f = [float(x) for x in t.view(F)]
    v0, e1, e2 = f[0:3], f[3:6], f[6:9]
    n, w, fine, sum_w = [], [], True, 0.0
    for a in range(3):
        b, c = (a + 1) % 3, (a + 2) % 3
        n.append(_f32(e1[b] * e2[c] - e1[c] * e2[b]))
        wd = abs(e1[b] * e2[c]) + abs(e1[c] * e2[b])
        w.append(_up(_f32(wd)))
        fine = fine and wd < 2.0 ** 100
        sum_w += w[-1]
    kd = _up(_f32(2.0 ** -19 * 2.0 * sum_w + 2.0 ** -100)) if fine else float("inf")
    out = np.zeros(16, np.uint32)
    out[0:10] = np.array(v0 + n + w + [kd], F).view(np.uint32)
    out[0:3] = t[0:3]                       # (v0 is copied, whatever its bits)
    out[15] = t[15]
    return out


# ---- the record comparisons: name -> (open(rtx, samples) -> scene, pose, two eyes) ------------------------------------------
def record_cases(rtx, orc, samples):
    """the scenes whose device planes and posed aimed stream are compared with the host statement: the bunny under `tilt`
    (ground moved) and `turn`, the lifted ground, a soup with the ground, a soup without a global triangle, and a brute-force
    scene, which aims nothing"""
    import os
    bunny = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "models", "big_bunny.obj")
    small = ps.small_scenes(rtx)
    side, back = vs.BUNNY_VIEWS["side"][1], vs.BUNNY_VIEWS["back"][1]

    def open_bunny():
        return rtx.default_scene([bunny], qs.W, qs.H, samples)

    out = {
        "tilt": (open_bunny, ps.bunny_pose(orc, "tilt"), (side, back)),
        "turn": (open_bunny, ps.bunny_pose(orc, "turn"), (side, back)),
        "lifted": (lambda: lift_scene(rtx, samples), lift_pose(), (LIFT_VIEW[1], (-30.0, 25.0, 80.0))),
    }
    for name in ("soup257_ground", "soup256", "soup255_brute"):
        sc = small[name]
        out[name] = ((lambda sc=sc: ps.open_small(rtx, samples, sc)), sc[4], ((0.0, 100.0, 200.0), (-80.0, 150.0, -40.0)))
    return out
