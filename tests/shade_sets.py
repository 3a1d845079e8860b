"""Ray sets for the rtx_shade_rays tests, with the CPU oracle's answers: numpy and the oracle binding only, no GPU.

oracle_shade is render_pixel (main.rs:180-240) composed from oracle PIECES — orc_closest_hit for the primary and the
shadow ray, orc_triangle_get_sample for the light point, orc_ray_new for Ray::new, orc_triangle_new for a triangle's
normal — with the arithmetic between them (lnd, the two distances, the ordered sum) in float32 numpy through np_ref's
_dot / _norm / _sub.  tests/test_shade_sets.py pins it, without a GPU, against the oracle's own render_pixel
(orc_render_rows_ex) and states the conditions the sets must meet; tests/test_gpu_shade_rays.py shades the sets.
Every set is built once per process."""
import ctypes as C

import numpy as np

import np_ref
import query_sets as qs
from query_sets import F, H, NO_HIT, W

SHADE_DTYPE = np.dtype([("linear", np.float32, 3), ("rgb8", np.uint8, 3), ("hits", np.uint8)])
PENUMBRA_POINTS = 128
PENUMBRA_FROM, PENUMBRA_TO = (-270.0, 40.0), (-140.0, 40.0)     # (x, z) on the ground: lit at one end, in the umbra at the other


def prim_tables(orc, tris, rgb, spheres=None, sphere_rgb=None, kinds=None):
    """per position in the Vec<Primitive>: colour, a triangle's normal by orc_triangle_new (a sphere's row: its origin),
    and whether it is a sphere"""
    tris = np.ascontiguousarray(tris, F).reshape(-1, 9)
    rgb = np.ascontiguousarray(rgb, F).reshape(-1, 3)
    n_s = 0 if spheres is None else len(spheres)
    if kinds is None:
        kinds = np.concatenate([np.zeros(len(tris), np.uint8), np.ones(n_s, np.uint8)])
    colour, normal = np.zeros((len(kinds), 3), F), np.zeros((len(kinds), 3), F)
    e1, e2 = np.zeros(3, F), np.zeros(3, F)
    it = isp = 0
    for k, kind in enumerate(kinds):
        if kind == 0:
            t = tris[it]
            n = np.zeros(3, F)
            orc.lib().orc_triangle_new(orc._fp(t[0:3].copy()), orc._fp(t[3:6].copy()), orc._fp(t[6:9].copy()),
                                       orc._fp(e1), orc._fp(e2), orc._fp(n))
            colour[k], normal[k] = rgb[it], n
            it += 1
        else:
            colour[k], normal[k] = sphere_rgb[isp], spheres[isp, :3]
            isp += 1
    return dict(rgb=colour, normals=normal, sphere=np.asarray(kinds) == 1)


def light_points(orc, light_tri, samples, nb_ray, nb_light):
    """[nb_ray, nb_light, 3]: Light::get_sample(T[(r*nb_ray + i) % n]) (main.rs:194-196)"""
    lt = np.ascontiguousarray(light_tri, F).reshape(9)
    out = np.zeros((nb_ray, nb_light, 3), F)
    for r in range(nb_ray):
        for i in range(nb_light):
            s = samples[(r * nb_ray + i) % len(samples)]
            orc.lib().orc_triangle_get_sample(orc._fp(lt[0:3].copy()), orc._fp(lt[3:6].copy()), orc._fp(lt[6:9].copy()),
                                              float(s[0]), float(s[1]), orc._fp(out[r, i]))
    return out


def units_of(orc, directions):
    """Ray::new (ray.rs:12-17) by the oracle, per direction"""
    return np.stack([qs.unit(orc, d) for d in np.ascontiguousarray(directions, F).reshape(-1, 3)]) if len(directions) \
        else np.zeros((0, 3), F)


def _closest(osc, origins, units):
    prim = np.full(len(origins), NO_HIT, np.uint32)
    t, p = np.zeros(len(origins), F), np.zeros((len(origins), 3), F)
    for k in range(len(origins)):
        h = osc.closest_hit(origins[k], units[k])
        if h.hit:
            prim[k], t[k], p[k] = h.tri, h.t, list(h.p_hit)
    return prim, t, p


def oracle_shade(orc, osc, origins, unit_dirs, nb_ray, nb_light, light_tri, samples, rgb, normals, sphere=None):
    """render_pixel where create_rays returns Ray{origins[p*nb_ray + r], unit_dirs[p*nb_ray + r]}.  rgb / normals / sphere:
    prim_tables' arrays.  -> dict(shade = SHADE_DTYPE records, lit = lit samples per pixel, samples = shadow rays per
    pixel, hit = qs.HIT_DTYPE records of the primary rays (normal left zero))"""
    origins = np.ascontiguousarray(origins, F).reshape(-1, 3)
    unit_dirs = np.ascontiguousarray(unit_dirs, F).reshape(-1, 3)
    assert len(origins) % nb_ray == 0
    n = len(origins) // nb_ray
    if sphere is None:
        sphere = np.zeros(len(rgb), bool)
    lp = light_points(orc, light_tri, samples, nb_ray, nb_light)
    denom = F(nb_ray * nb_light)                                                    # main.rs:211
    avg = np.zeros((n, 3), F)
    hits, lit_count = np.zeros(n, np.int64), np.zeros(n, np.int64)
    rec = np.zeros(len(origins), qs.HIT_DTYPE)
    rec["prim"] = NO_HIT
    for r in range(nb_ray):
        o, d = origins[r::nb_ray], unit_dirs[r::nb_ray]
        prim, t, p_hit = _closest(osc, o, d)                                        # main.rs:187
        rec["prim"][r::nb_ray], rec["t"][r::nb_ray], rec["p_hit"][r::nb_ray] = prim, t, p_hit
        hp = np.nonzero(prim != NO_HIT)[0]
        if not len(hp):
            continue
        hits[hp] += 1
        orig = p_hit[hp]                                                            # main.rs:192
        colour = rgb[prim[hp]]                                                      # main.rs:191
        normal = normals[prim[hp]].copy()                                           # bvh.rs:72
        sp = sphere[prim[hp]]
        if sp.any():                                                                # sphere.rs:93-95
            normal[sp] = np.stack(np_ref._normalize(np_ref._sub(np_ref._v(orig[sp]), np_ref._v(normal[sp]))), axis=-1)
        for i in range(nb_light):                                                   # main.rs:193
            to_light = np.stack(np_ref._sub(np_ref._v(lp[r, i]), np_ref._v(orig)), axis=-1).astype(F)   # p - orig
            sd = units_of(orc, to_light)                                            # main.rs:201 -> ray.rs:15
            dist_to_light = np_ref._norm(np_ref._v(to_light))                       # main.rs:202
            sprim, _, sp_hit = _closest(osc, orig, sd)                              # main.rs:204
            lnd = np.abs(np_ref._dot(np_ref._v(normal), np_ref._v(sd)))             # main.rs:207
            dist_hit = np_ref._norm(np_ref._sub(np_ref._v(orig), np_ref._v(sp_hit)))
            lit = (sprim == NO_HIT) | (dist_hit > dist_to_light)                    # main.rs:218-232
            for c in range(3):
                term = np.where(lit, (colour[:, c] * lnd) / denom, (F(0.0) * F(1.0)) / denom)   # main.rs:211-215, :226
                avg[hp, c] = avg[hp, c] + term
            lit_count[hp] += lit
    shade = np.zeros(n, SHADE_DTYPE)
    shade["linear"] = avg
    byte = np.zeros(3, np.uint8)
    for k in range(n):
        orc.lib().orc_color_to_rgb8(orc._fp(avg[k]), byte.ctypes.data_as(C.POINTER(C.c_uint8)))      # color.rs:28-33
        shade["rgb8"][k] = byte
    shade["hits"] = np.minimum(hits, 255)
    return dict(shade=shade, lit=lit_count, samples=hits * nb_light, hit=rec)


def shade_set(orc, osc, origins, directions, nb_ray, nb_light, light_tri, samples, tables):
    """a set: the caller's rays (directions of any length) and the oracle's answer for Ray::new of them"""
    origins = np.ascontiguousarray(origins, F).reshape(-1, 3)
    directions = np.ascontiguousarray(directions, F).reshape(-1, 3)
    units = units_of(orc, directions)
    out = oracle_shade(orc, osc, origins, units, nb_ray, nb_light, light_tri, samples, tables["rgb"], tables["normals"],
                       tables["sphere"])
    out.update(origins=origins, directions=directions, units=units, nb_ray=nb_ray)
    return out


def take(s, pixels):
    """the named pixels of a set (per-pixel results do not depend on the other pixels)"""
    pixels = np.asarray(pixels)
    nb = s["nb_ray"]
    rays = (pixels[:, None] * nb + np.arange(nb)[None, :]).reshape(-1)
    out = dict(nb_ray=nb)
    for k in ("shade", "lit", "samples"):
        out[k] = s[k][pixels]
    for k in ("hit", "origins", "directions", "units"):
        out[k] = s[k][rays]
    return out


def join(*sets):
    out = dict(nb_ray=sets[0]["nb_ray"])
    for k in ("shade", "lit", "samples", "hit", "origins", "directions", "units"):
        out[k] = np.concatenate([s[k] for s in sets])
    return out


def camera_raw_rays(orc, width, height, eye, look_at, up, distance, samples, nb_ray=1):
    """create_rays' arithmetic (main.rs:151-178) up to, and not including, normalize, in float32 as np_ref.primary_rays has
    it; pixel k = py * width + px (the frame's byte order, put_pixel main.rs:293-294), its rays consecutive"""
    u, v, w = (np.zeros(3, F) for _ in range(3))
    orc.lib().orc_camera_new(orc._fp(orc.f3(eye)), orc._fp(orc.f3(look_at)), orc._fp(orc.f3(up)), orc._fp(u), orc._fp(v), orc._fp(w))
    py, px = np.divmod(np.arange(width * height, dtype=np.uint32), np.uint32(width))
    d = np.zeros((width * height, nb_ray, 3), F)
    for i in range(nb_ray):
        k = (px * np.uint32(width) + py + np.uint32(i)) % np.uint32(len(samples))   # :162,165 (u32)
        a = px.astype(F) - F(width) / F(2.0) + samples[k, 0]
        b = py.astype(F) - F(height) / F(2.0) + samples[k, 1]
        for c in range(3):
            d[:, i, c] = (a * u[c] + b * v[c]) - F(distance) * w[c]
    o = np.broadcast_to(np.asarray(eye, F), (width * height * nb_ray, 3)).copy()
    return o, d.reshape(-1, 3), (u, v, w), px, py


def penumbra_line():
    """(c): ground points on a line across the boundary of the bunny's shadow — from the lit ground beside it, through the
    penumbra, into the umbra — each looked at from 50 units above by a ray leaning slightly off the vertical"""
    s = np.linspace(0.0, 1.0, PENUMBRA_POINTS)
    ground = np.stack([PENUMBRA_FROM[0] + s * (PENUMBRA_TO[0] - PENUMBRA_FROM[0]), np.zeros_like(s),
                       PENUMBRA_FROM[1] + s * (PENUMBRA_TO[1] - PENUMBRA_FROM[1])], axis=1)
    d = np.tile(np.array([0.03, -1.0, 0.02]), (PENUMBRA_POINTS, 1))
    return (ground - 50.0 * d).astype(F), (d * 7.0).astype(F)


def bunny_sets(orc, samples):
    """(a) camera, (b) random, (c) penumbra, (e) hard ray, (f) far origin on big_bunny + ground"""
    def make():
        b = qs.bunny(orc, samples)
        osc = b["osc"]
        tables = prim_tables(orc, osc.tris, osc.rgb)
        args = (1, orc.NB_LIGHT_SAMPLE, orc.LIGHT_TRI, samples, tables)
        out = dict(osc=osc, tables=tables)
        o, d, cam, px, py = camera_raw_rays(orc, W, H, orc.EYE, orc.LOOK_AT, orc.UP, orc.DISTANCE, samples)
        out["camera"] = shade_set(orc, osc, o, d, *args)
        out["camera"].update(cam=cam, px=px, py=py)
        ro, rd, _, _ = b["sets"]["random"]
        out["random"] = shade_set(orc, osc, ro[:256], rd[:256], *args)
        out["penumbra"] = shade_set(orc, osc, *penumbra_line(), *args)
        first63 = take(out["random"], np.arange(63))
        ho, hd = (np.array([v], F) for v in qs.HARD_RAYS["x"])
        out["hard"] = join(first63, shade_set(orc, osc, ho, hd, *args))
        out["hard_twin"] = shade_set(orc, osc, ho, qs.positive_twin(hd[0])[None], *args)
        fo, ft = qs.far_origin_ray()
        out["far"] = join(first63, shade_set(orc, osc, fo[None], (ft - fo).astype(F)[None], *args))
        return out
    return qs._once("shade_bunny", make)


def soup_sets(orc, samples):
    """(d): 192 of set A's pairs as rays on scene A (220 triangles, 60 spheres), as 192 pixels of one ray and as 96 pixels
    of two (an oracle scene of the same soup with nb_ray = 2: the light points of ray 1 are other table entries)"""
    def make():
        a = qs.scene_a(orc, samples)
        so, sd, _, _ = qs.set_a(orc, samples)["trace"]
        Wd, Hd, tris, rgb, _ = a["args"]
        kw = a["kw"]
        tables = prim_tables(orc, tris, rgb, kw["spheres"], kw["sphere_rgb"], kw["kinds"])
        nb_light, light = kw["nb_light_sample"], kw["light_tri"]
        out = dict(a=a, tables=tables)
        out[1] = shade_set(orc, a["osc"], so[:192], sd[:192], 1, nb_light, light, samples, tables)
        osc2 = orc.Scene(Wd, Hd, tris, rgb, samples, nb_ray=2, **kw)
        out["osc2"] = osc2
        out[2] = shade_set(orc, osc2, so[:192], sd[:192], 2, nb_light, light, samples, tables)
        return out
    return qs._once("shade_soup", make)


def classes(s):
    """per pixel: 0 all rays miss, 1 every sample lit, 2 every sample occluded, 3 some of each"""
    c = np.full(len(s["shade"]), 3)
    c[s["lit"] == s["samples"]] = 1
    c[s["lit"] == 0] = 2
    c[s["shade"]["hits"] == 0] = 0
    return c
