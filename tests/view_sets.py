"""Views for the rtx_render_view tests, with the CPU oracle's answers: numpy and the oracle binding only, no GPU.

A view of an uploaded scene has two independent expected values:
    composition   shade_sets.shade_set on shade_sets.camera_raw_rays' rays of the view, traced against the oracle scene
                  created with ANOTHER camera (the scene the library has uploaded): render_pixel from oracle pieces
    oracle scene  an oracle scene created WITH the view's frame and camera, rendered by the oracle's own render_pixel
tests/test_view_sets.py asserts, without a GPU, that the two agree and that the views hold what they are for;
tests/test_gpu_render_view.py renders them.  Everything is built once per process (query_sets._once).

The bunny views are on big_bunny + ground as query_sets.bunny holds it (32 x 32, default camera, seeded table); the soup
view on query_sets.scene_a's soup at nb_ray = 2 (shade_sets.soup_sets' osc2)."""
import numpy as np

import query_sets as qs
import sequence_sets as sq
import shade_sets as ss
from query_sets import F, NO_HIT

UP = (0.0, 1.0, 0.0)
# name: frame (width, height), eye, look_at, distance
BUNNY_VIEWS = {
    "side": ((44, 27), (320.0, 140.0, 40.0), (-20.0, 70.0, 0.0), 30.0),
    "back": ((35, 30), (-60.0, 260.0, -330.0), (-15.0, 40.0, 0.0), 26.0),
    "far": ((21, 19), (3000.0, 9000.0, 30000.0), (-15.0, 60.0, 0.0), 1500.0),
}
SOUP_VIEW = ((29, 22), (7.0, 5.0, 9.0), (0.0, 0.0, -22.0), 22.0)
SCENE_BOUND = 10000.0                      # the ground's largest coordinate: beyond it an origin is out of the fast test's range
SIDE_RECTS = ((5, 3, 19, 13), (8, 8, 16, 8), (0, 0, 1, 1), (43, 26, 1, 1), (0, 26, 44, 1))     # (x0, y0, nx, ny)
# four eyes on a circle around the bunny, 24 x 16 each
TURNTABLE_FRAME, TURNTABLE_LOOK_AT, TURNTABLE_DISTANCE = (24, 16), (-15.0, 90.0, 0.0), 14.0
TURNTABLE_EYES = tuple((float(-15.0 + 300.0 * np.cos(a)), 150.0, float(300.0 * np.sin(a))) for a in np.deg2rad((20.0, 110.0, 200.0, 290.0)))
# the scenes of test 4 are created with this camera and rendered through their descriptions' own
HARD_CREATED = dict(width=16, height=16, eye=(1.0, 30.0, 22.0), look_at=(0.0, 0.0, -14.0), distance=24.0)


def camera(v):
    """keywords both bindings' Scene and rtx.Scene.view take"""
    return dict(eye=v[1], look_at=v[2], up=UP, distance=v[3])


def _view(orc, osc_uploaded, osc_view, v, nb_ray, nb_light, light_tri, samples, tables, want_planes):
    (w, h), eye, look_at, distance = v
    o, d, cam, px, py = ss.camera_raw_rays(orc, w, h, eye, look_at, UP, distance, samples, nb_ray)
    s = ss.shade_set(orc, osc_uploaded, o, d, nb_ray, nb_light, light_tri, samples, tables)
    s.update(cam=cam, px=px, py=py)
    if want_planes:
        frame, st, tri, lin = osc_view.render_rows(mode=orc.MODE_BVH, want_tri=True, want_lin=True)
    else:                                  # (the planes hold one ray's hit per pixel)
        frame, st = osc_view.render_rows(mode=orc.MODE_BVH)
        tri = lin = None
    frame.setflags(write=False)
    return dict(v=v, w=w, h=h, nb_ray=nb_ray, set=s, osc=osc_view, frame=frame, stats=st, tri=tri, lin=lin)


def bunny_view(orc, samples, name):
    """-> dict(v, w, h, set = the composition on the 32 x 32 default-camera oracle scene (shade, hit, origins, directions,
    lit, samples, px, py), osc / frame / stats / tri / lin = the oracle scene created with the view's camera, rendered)"""
    def make():
        b = ss.bunny_sets(orc, samples)
        v = BUNNY_VIEWS[name]
        osc = orc.default_scene(["big_bunny.obj"], v[0][0], v[0][1], samples, **camera(v))
        return _view(orc, b["osc"], osc, v, 1, orc.NB_LIGHT_SAMPLE, orc.LIGHT_TRI, samples, b["tables"], True)
    return qs._once("view_" + name, make)


def soup_view(orc, samples):
    """the same on scene A's soup with two rays per pixel; `a`: query_sets.scene_a"""
    def make():
        sets = ss.soup_sets(orc, samples)
        a = sets["a"]
        _, _, tris, rgb, _ = a["args"]
        kw = dict(a["kw"], **camera(SOUP_VIEW))
        osc = orc.Scene(SOUP_VIEW[0][0], SOUP_VIEW[0][1], tris, rgb, samples, nb_ray=2, **kw)
        out = _view(orc, sets["osc2"], osc, SOUP_VIEW, 2, a["kw"]["nb_light_sample"], a["kw"]["light_tri"], samples,
                    sets["tables"], False)
        out["a"] = a
        return out
    return qs._once("view_soup", make)


def window(view, rect):
    """the rectangle's slice of a whole view's per-pixel arrays: (frame bytes, shade records, hit records [ny, nx, nb_ray])"""
    x0, y0, nx, ny = rect
    w, h, nb = view["w"], view["h"], view["nb_ray"]
    ys, xs = slice(y0, y0 + ny), slice(x0, x0 + nx)
    return (view["frame"][ys, xs], view["set"]["shade"].reshape(h, w)[ys, xs], view["set"]["hit"].reshape(h, w, nb)[ys, xs])


def turntable(orc, samples):
    """[(view tuple, the oracle scene's frame, its statistics)] for TURNTABLE_EYES"""
    def make():
        out = []
        for eye in TURNTABLE_EYES:
            v = (TURNTABLE_FRAME, eye, TURNTABLE_LOOK_AT, TURNTABLE_DISTANCE)
            osc = orc.default_scene(["big_bunny.obj"], v[0][0], v[0][1], samples, **camera(v))
            frame, st = osc.render_rows(mode=orc.MODE_BVH)
            out.append((v, frame, st))
        return out
    return qs._once("view_turntable", make)


def hard_scene(name, orc, samples, rtx=None):
    """P or S of sequence_sets: dict(ref = sequence_sets.reference(name) — the oracle's frame through the description's own
    camera —, created = keywords of a scene with the same primitives, table, nb_ray and nb_light_sample made with
    HARD_CREATED's frame and camera, v = the description's own frame and camera as a view tuple)"""
    ref = sq.reference(name, orc, samples, rtx)
    d = ref["desc"]
    kw = dict(d["kw"], eye=HARD_CREATED["eye"], look_at=HARD_CREATED["look_at"], distance=HARD_CREATED["distance"])
    v = ((d["W"], d["H"]), d["kw"]["eye"], d["kw"]["look_at"], d["kw"]["distance"])
    return dict(ref=ref, args=(HARD_CREATED["width"], HARD_CREATED["height"]) + tuple(d["args"]), kw=kw, v=v)


def neg_zero_tiles(ref):
    """8 x 8 tiles of the whole frame that hold a primary ray with a -0.0 direction component, and those rays"""
    return sq.tiles_holding_a_hard_ray(ref, 0, ref["desc"]["H"]), int(ref["neg_zero"].sum())


def sphere_rays(view):
    return int(qs.is_sphere(view["a"], view["set"]["hit"]).sum())

