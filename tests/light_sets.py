"""Lights for the relighting tests (rtx_render_view_lit, rtx_shade_rays_lit), with the CPU oracle's answers: numpy and the
oracle binding only, no GPU.

A frame under another light has the two independent expected values a view has (view_sets.py):
    composition   shade_sets.shade_set on the view's rays with the OTHER light and sample count, traced against the oracle
                  scene the library has uploaded: render_pixel from oracle pieces.  It needs no new oracle scene, so every
                  fixture has it
    oracle scene  an oracle scene created with the view's camera AND the light and count, rendered by the oracle's own
                  render_pixel.  Each repeats the oracle's O(n^2) tree build: three exist on big_bunny — the "side" view
                  under the moved light, two lights of the orbit — and the composition is pinned to them
tests/test_light_sets.py asserts, without a GPU, that the two agree and that the fixtures hold what they are for;
tests/test_gpu_relight.py renders them.  Everything is built once per process (query_sets._once).

The bunny fixtures are on big_bunny + ground as query_sets.bunny holds it (32 x 32, default camera, seeded table), seen
through view_sets' "side" view (44 x 27) or the turntable's first eye (24 x 16); the soup fixture on query_sets.scene_a's
soup at nb_ray = 2 through view_sets.SOUP_VIEW.  The sample counts are kept small where nothing asks for 100: a
composition costs one oracle call per shadow ray."""
import numpy as np

import query_sets as qs
import shade_sets as ss
import view_sets as vs

# name: (v0, v1, v2 of Light.primitives[0], NB_LIGHT_SAMPLE).  The scene's own light is a 20-unit triangle at y = 300 above
# the bunny; the side view looks from +x.
SIDE_LIGHTS = {
    # (a) moved to the far side of the bunny (seen from the side view's eye): the ground shadow falls towards the camera
    "far_side": ((-270.0, 260.0, -25.0, -230.0, 260.0, -25.0, -250.0, 265.0, 25.0), 100),
    # (b) low over the ground: long shadows, |normal . direction| small on the ground
    "grazing": ((-30.0, 22.0, 330.0, 30.0, 22.0, 330.0, 0.0, 52.0, 330.0), 40),
    # (c) 30,000 units away, beyond view_sets.SCENE_BOUND, and as wide in angle as the scene's own
    "distant": ((1500.0, 30000.0, 9000.0, 4500.0, 30000.0, 9000.0, 3000.0, 30000.0, 12000.0), 50),
    # (d) a point light: every sample is the one vertex
    "point": ((-120.0, 280.0, 90.0, -120.0, 280.0, 90.0, -120.0, 280.0, 90.0), 16),
}
PARTLY_LIT = ("far_side", "grazing", "distant")
OWN_COUNTS = (1, 7, 130)                   # (e) the scene's own triangle: one sample, a few, more than rtx_scene_create's 100
WRAP_PAIRS, WRAP_COUNT = 5, 12             # (f) a sample table of fewer pairs than the count: (r*nb_ray + i) % n_samples wraps
SOUP_LIGHT = ((-9.0, 6.0, -8.0, -7.0, 7.0, -10.0, -8.0, 9.0, -6.0), 0)      # count 0: the scene's own 24
ORBIT_COUNT = 32
ORBIT_LIGHTS = tuple((float(-15.0 + 260.0 * np.cos(a)) - 12.0, 270.0, float(260.0 * np.sin(a)) - 12.0,
                      float(-15.0 + 260.0 * np.cos(a)) + 12.0, 270.0, float(260.0 * np.sin(a)) - 12.0,
                      float(-15.0 + 260.0 * np.cos(a)), 290.0, float(260.0 * np.sin(a)) + 12.0)
                     for a in np.deg2rad((35.0, 125.0, 215.0, 305.0)))
ORBIT_ORACLE = (0, 2)                      # the orbit's lights that have an oracle scene
ORBIT_VIEW = (vs.TURNTABLE_FRAME, vs.TURNTABLE_EYES[0], vs.TURNTABLE_LOOK_AT, vs.TURNTABLE_DISTANCE)
MAX_POINTS = 1 << 20                       # nb_ray * count of one lit call


def points(orc, light_tri, samples, nb_ray, count):
    """[nb_ray * count, 3]: get_sample(T[(r*nb_ray + i) % n]) by the oracle (shade_sets.light_points)"""
    return ss.light_points(orc, light_tri, samples, nb_ray, count).reshape(-1, 3)


def relit(orc, osc_uploaded, v, nb_ray, light_tri, count, samples, tables):
    """the composition of view tuple v under (light_tri, count) -> dict(v, w, h, nb_ray, light, count, set, frame [h, w, 3])"""
    (w, h), eye, look_at, distance = v
    o, d, _, _, _ = ss.camera_raw_rays(orc, w, h, eye, look_at, vs.UP, distance, samples, nb_ray)
    s = ss.shade_set(orc, osc_uploaded, o, d, nb_ray, count, light_tri, samples, tables)
    frame = np.ascontiguousarray(s["shade"]["rgb8"].reshape(h, w, 3))
    frame.setflags(write=False)
    return dict(v=v, w=w, h=h, nb_ray=nb_ray, light=tuple(light_tri), count=count, set=s, frame=frame)


def oracle_frame(orc, v, light_tri, count, samples):
    """(frame, statistics) of an oracle scene created with the view's camera, the light and the count"""
    osc = orc.default_scene(["big_bunny.obj"], v[0][0], v[0][1], samples, light_tri=light_tri, nb_light_sample=count,
                            **vs.camera(v))
    frame, st = osc.render_rows(mode=orc.MODE_BVH)
    osc.close()
    frame.setflags(write=False)
    return frame, st


def side(orc, samples, name):
    """"side" under SIDE_LIGHTS[name]; "far_side" also carries oracle = (frame, statistics) of its oracle scene"""
    def make():
        b = ss.bunny_sets(orc, samples)
        tri, count = SIDE_LIGHTS[name]
        out = relit(orc, b["osc"], vs.BUNNY_VIEWS["side"], 1, tri, count, samples, b["tables"])
        out["oracle"] = oracle_frame(orc, out["v"], tri, count, samples) if name == "far_side" else None
        return out
    return qs._once("light_side_" + name, make)


def side_count(orc, samples, count):
    """(e): "side" under the scene's own triangle with another count"""
    def make():
        b = ss.bunny_sets(orc, samples)
        return relit(orc, b["osc"], vs.BUNNY_VIEWS["side"], 1, orc.LIGHT_TRI, count, samples, b["tables"])
    return qs._once("light_side_count_%d" % count, make)


def side_wrap(orc, samples):
    """(f): "side" of a scene whose table is the first WRAP_PAIRS pairs, under the moved light with WRAP_COUNT samples"""
    def make():
        b = ss.bunny_sets(orc, samples)                    # (orc_closest_hit does not read the table)
        short = np.ascontiguousarray(samples[:WRAP_PAIRS])
        out = relit(orc, b["osc"], vs.BUNNY_VIEWS["side"], 1, SIDE_LIGHTS["far_side"][0], WRAP_COUNT, short, b["tables"])
        out["samples"] = short
        return out
    return qs._once("light_side_wrap", make)


def soup(orc, samples):
    """view_sets.soup_view's view (spheres, nb_ray = 2: ray 1 reads table entries 2 + i) under SOUP_LIGHT; `a`: query_sets.scene_a"""
    def make():
        sets = ss.soup_sets(orc, samples)
        a = sets["a"]
        count = SOUP_LIGHT[1] or a["kw"]["nb_light_sample"]
        out = relit(orc, sets["osc2"], vs.SOUP_VIEW, 2, SOUP_LIGHT[0], count, samples, sets["tables"])
        out["a"] = a
        return out
    return qs._once("light_soup", make)


def orbit(orc, samples):
    """[composition of ORBIT_VIEW under ORBIT_LIGHTS[k], ORBIT_COUNT samples], those of ORBIT_ORACLE with oracle = (frame,
    statistics)"""
    def make():
        b = ss.bunny_sets(orc, samples)
        out = []
        for k, tri in enumerate(ORBIT_LIGHTS):
            r = relit(orc, b["osc"], ORBIT_VIEW, 1, tri, ORBIT_COUNT, samples, b["tables"])
            r["oracle"] = oracle_frame(orc, ORBIT_VIEW, tri, ORBIT_COUNT, samples) if k in ORBIT_ORACLE else None
            out.append(r)
        return out
    return qs._once("light_orbit", make)


def partly_lit(s):
    """pixels of a composition with 0 < lit samples < shadow rays"""
    return int(((s["lit"] > 0) & (s["lit"] < s["samples"])).sum())
