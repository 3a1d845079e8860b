"""Fixtures for the tests of rtx_render_view_rows_shade that the other fixture modules do not hold, with the CPU oracle's
answers: numpy and the oracle binding only, no GPU.

    ODD_SIDE        lit_rows_sets.SIDE in a 43 x 29 frame: a width that is no multiple of the tile's 8 (five whole tiles and
                    three columns of a sixth) and a height that is none either
    yard_hit_counts per pixel of accum_sets.YARD_MEAN_VIEW over the uploaded yard, how many of its two rays have a closest hit
    hit_mask        per pixel of a bunny view, whether its one ray has a closest hit
tests/test_rows_shade_sets.py asserts the conditions the GPU tests rely on.  Everything is built once per process
(query_sets._once) and read-only."""
import numpy as np

import accum_sets as ac
import lit_rows_sets as lr
import prims_sets as pm
import query_sets as qs
import resample_sets as rs
import shade_sets as ss
import view_sets as vs
from query_sets import NO_HIT

ODD_FRAME = (43, 29)
ODD_SIDE = (ODD_FRAME,) + tuple(lr.SIDE[1:])
WINDOW = (3, 13)                      # rows [3, 16): a start off the tile grid, a height that is no multiple of 8


def hit_mask(orc, samples, v):
    """bool [h, w]: the oracle's closest hit of the one ray per pixel of big_bunny + ground seen through view tuple v"""
    def make():
        osc = orc.default_scene(["big_bunny.obj"], v[0][0], v[0][1], samples, **vs.camera(v))
        _, _, tri = osc.render_rows(mode=orc.MODE_BVH, want_tri=True)
        osc.close()
        out = tri != NO_HIT
        out.setflags(write=False)
        return out
    return qs._once("rows_shade_hit_mask_%r" % (v,), make)


def yard_hit_counts(orc, rtx, samples):
    """uint8 [h, w]: rays with a closest hit, of the two per pixel, of the uploaded yard through accum_sets.YARD_MEAN_VIEW"""
    def make():
        (w, h), eye, look_at, distance = ac.YARD_MEAN_VIEW
        table = samples[:4096]                                     # prims_sets.open_yard's table
        osc = rs.yard_oracle(orc, pm.yard(rtx), table, **vs.camera(ac.YARD_MEAN_VIEW))
        o, d, _, _, _ = ss.camera_raw_rays(orc, w, h, eye, look_at, vs.UP, distance, table, pm.NB_RAY)
        exp, _ = qs.oracle_hits(orc, osc, o, d, qs.HIT_DTYPE)
        osc.close()
        out = (exp["prim"] != NO_HIT).reshape(h, w, pm.NB_RAY).sum(axis=2).astype(np.uint8)
        out.setflags(write=False)
        return out
    return qs._once("rows_shade_yard_hit_counts", make)


def tiles_with_both(mask, least=10):
    """8 x 8 tiles of a hit mask that hold at least `least` pixels with a hit and `least` without"""
    h, w = mask.shape
    out = []
    for ty in range(0, h, 8):
        for tx in range(0, w, 8):
            t = mask[ty:ty + 8, tx:tx + 8]
            if t.sum() >= least and (~t).sum() >= least:
                out.append((tx // 8, ty // 8))
    return out
