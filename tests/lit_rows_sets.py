"""Frames for the tests of rtx_render_view_rows_lit (any view under any light through the render pipeline), with the CPU
oracle's answers: numpy and the oracle binding only, no GPU.  light_sets and view_sets are used as they are.

A lit pipeline frame has light_sets' two expected values:
    oracle scene  light_sets.oracle_frame: an oracle scene created with the view's camera, the light and the count
    composition   light_sets.relit: render_pixel from oracle pieces on the view's rays with that light — what
                  rtx_render_view_lit is tested against
The four side lights, the own triangle at 1 / 129 / 257 samples and two lights of the orbit have the first; the rest the
second.  tests/test_lit_rows_host.py asserts, without a GPU, that the fixtures hold what they are for;
tests/test_gpu_lit_rows.py renders them.  Everything is built once per process (query_sets._once).

big_bunny + ground as query_sets.bunny holds it (created 32 x 32, default camera, seeded table) is seen through 48 x 32
frames — six tiles by four, more than one workgroup of every pipeline kernel — of view_sets' "side" camera and of the
turntable's first eye; the soup is light_sets.soup's (spheres, nb_ray = 2, 29 x 22).

The counts sit at the tour kernel's edges (a batch is 128 samples): 1 and 2 have no 2-opt, 3 is the least that has, 128 is
one full batch, 129 a second batch of one point, 130 of two, 257 three batches."""
import numpy as np

import light_sets as ls
import query_sets as qs
import shade_sets as ss
import view_sets as vs

FRAME = (48, 32)
SIDE = (FRAME,) + tuple(vs.BUNNY_VIEWS["side"][1:])
TURN = (FRAME, vs.TURNTABLE_EYES[0], vs.TURNTABLE_LOOK_AT, 2.0 * vs.TURNTABLE_DISTANCE)     # (twice the frame: twice the distance)
COUNTS = (1, 2, 3, 7, 100, 128, 129, 130, 257)
ORACLE_COUNTS = (1, 129, 257)              # the own triangle's counts that have an oracle scene
BATCH = 128
# finite vertices so large that the squares behind every distance overflow (and some points do): no distance ever wins
OVERFLOW_LIGHTS = ((3e38, 3e38, 3e38, -3e38, 3e38, -3e38, 3e38, -3e38, 3e38),
                   (3.4e38, 0.0, 0.0, 3.4e38, 3.4e38, 0.0, -3.4e38, 0.0, 3.4e38))


def _fixture(v, nb_ray, tri, count, frame, stats=None, composed=None, **more):
    frame.setflags(write=False)
    return dict(v=v, w=v[0][0], h=v[0][1], nb_ray=nb_ray, light=tuple(tri), count=count, frame=frame, stats=stats,
                set=composed, **more)


def by_oracle(orc, samples, v, tri, count):
    frame, st = ls.oracle_frame(orc, v, tri, count, samples)
    return _fixture(v, 1, tri, count, frame, stats=st)


def by_composition(orc, samples, v, tri, count, table=None):
    b = ss.bunny_sets(orc, samples)                        # (orc_closest_hit does not read the table)
    r = ls.relit(orc, b["osc"], v, 1, tri, count, samples if table is None else table, b["tables"])
    return _fixture(v, 1, tri, count, r["frame"], composed=r["set"])


def side(orc, samples, name):
    """SIDE under light_sets.SIDE_LIGHTS[name]: the oracle scene created with that light"""
    tri, count = ls.SIDE_LIGHTS[name]
    return qs._once("lit_rows_side_" + name, lambda: by_oracle(orc, samples, SIDE, tri, count))


def side_composed(orc, samples, name):
    """the same frame by composition (the host test pins the two to each other and counts the partly lit pixels)"""
    tri, count = ls.SIDE_LIGHTS[name]
    return qs._once("lit_rows_side_composed_" + name, lambda: by_composition(orc, samples, SIDE, tri, count))


def own(orc, samples, count):
    """SIDE under the scene's own triangle with `count` samples"""
    make = by_oracle if count in ORACLE_COUNTS else by_composition
    return qs._once("lit_rows_own_%d" % count, lambda: make(orc, samples, SIDE, orc.LIGHT_TRI, count))


def orbit(orc, samples):
    """[TURN under light_sets.ORBIT_LIGHTS[k], ORBIT_COUNT samples]: those of ORBIT_ORACLE by their oracle scene"""
    def make():
        return [(by_oracle if k in ls.ORBIT_ORACLE else by_composition)(orc, samples, TURN, tri, ls.ORBIT_COUNT)
                for k, tri in enumerate(ls.ORBIT_LIGHTS)]
    return qs._once("lit_rows_orbit", make)


def wrap(orc, samples):
    """SIDE of a scene whose table is the first WRAP_PAIRS pairs, under the far-side light with WRAP_COUNT samples: duplicate
    points, zero distances and ties in the tour"""
    def make():
        short = np.ascontiguousarray(samples[:ls.WRAP_PAIRS])
        return dict(by_composition(orc, samples, SIDE, ls.SIDE_LIGHTS["far_side"][0], ls.WRAP_COUNT, table=short), samples=short)
    return qs._once("lit_rows_wrap", make)


def soup(orc, samples):
    """light_sets.soup as it is: its view is full width"""
    return ls.soup(orc, samples)


def all_lights(orc):
    """(triangle, name) of every fixture light"""
    out = [(tri, name) for name, (tri, _) in ls.SIDE_LIGHTS.items()] + [(orc.LIGHT_TRI, "own"), (ls.SOUP_LIGHT[0], "soup")]
    return out + [(tri, "orbit %d" % k) for k, tri in enumerate(ls.ORBIT_LIGHTS)]


def batches(count):
    """(first sample, samples) of every batch"""
    return [(b0, min(count - b0, BATCH)) for b0 in range(0, count, BATCH)]


def tour_records(points, order, nb_ray, count):
    """the 16-byte records the tour kernel writes, as uint32 [nb_ray * count, 4], from the host's points and order"""
    pts = np.ascontiguousarray(points, np.float32).reshape(nb_ray, count, 3)
    order = np.asarray(order, np.uint32).reshape(nb_ray, count)
    out = np.zeros((nb_ray, count, 4), np.uint32)
    for r in range(nb_ray):
        out[r, :, :3] = pts[r, order[r]].view(np.uint32)
        out[r, :, 3] = order[r] % BATCH
    return out.reshape(-1, 4)


def path_length(points):
    p = np.asarray(points, np.float64)
    return float(np.sqrt(((p[1:] - p[:-1]) ** 2).sum(axis=1)).sum())


def tile_classes(descs, w, h):
    """(tiles finished by the scheduling pass, tiles with a non-empty cut) among the w x h frame's own tiles of
    rtx_debug_tile_descs' words (tiles are numbered by 8 x 8 blocks; numbers outside the frame are padding)"""
    d = np.asarray(descs, np.uint32).reshape(-1, 4)
    tiles_x, tiles_y = (w + 7) // 8, (h + 7) // 8
    blocks_x = (tiles_x + 7) // 8
    t = np.arange(len(d))
    x, y = (t // 64 % blocks_x) * 8 + t % 8, (t // 64 // blocks_x) * 8 + t % 64 // 8
    real = (x < tiles_x) & (y < tiles_y)
    return int(((d[:, 0] == 0xFFFFFFFF) & real).sum()), int(((((d[:, 2] >> 8) & 0xFF) != 0) & real).sum())
