"""The conditions the fixtures of tests/colour_sets.py must meet, asserted with the CPU oracle alone (no GPU): a ladder
entry that did not lie AT its gamma step, or a colour class no pixel sees, would let tests/test_gpu_colours.py pass
without testing what it says it tests.  Each test prints the counts behind its conditions (pytest -s shows them)."""
import importlib

import numpy as np
import pytest

import colour_sets as cs
from colour_sets import NO_HIT, bits_of, f32
from query_sets import F


@pytest.fixture(scope="module")
def rtx():
    return importlib.import_module("ray-tracer-rust_amd")


# ---------------------------------------------------------------------------------------------- 1: the ladder
def test_thresholds_by_bisection_are_the_librarys_table(rtx, orc, samples_half):
    thr = cs.thresholds(orc)
    with cs.ground_scene(rtx, samples_half, (0.5, 0.5, 0.5), 1) as s:
        lib = s.gamma_thresholds()
    assert np.array_equal(thr.view(np.uint32), np.asarray(lib, F).view(np.uint32))
    assert cs.ladder()["thresholds"] == [bits_of(t) for t in thr[1:]]
    for b in range(1, 256):
        assert cs.oracle_byte(orc, thr[b]) == b and cs.oracle_byte(orc, cs.below(thr[b])) == b - 1


def test_every_stored_grey_entry_lies_at_its_step_on_both_sides(orc, samples_seeded):
    thr = cs.thresholds(orc)
    grey = cs.ladder()["grey"]
    tri = cs.ground_render(orc, samples_seeded, (0.5, 0.5, 0.5), 1)[2]
    assert sorted(cs.LADDER_PIXELS) == sorted((int(x), int(y)) for y, x in np.argwhere(tri != NO_HIT))
    exact = {n: 0 for n in cs.LADDER_COUNTS}
    for count in cs.LADDER_COUNTS:
        assert sorted(e["step"] for e in grey if e["count"] == count) == list(range(1, 256)), "every step, once"
    for e in grey:
        (x, y), b = e["pixel"], e["step"]
        assert e["c_hi"] == e["c_lo"] + 1 and e["distance"] in cs.LADDER_DISTANCES
        for c, want_lin, want_byte in ((e["c_hi"], thr[b], b), (e["c_lo"], cs.below(thr[b]), b - 1)):
            frame, lin, _ = cs.ground_render(orc, samples_seeded, (f32(c),) * 3, e["count"], e["distance"])
            assert [bits_of(v) for v in lin[y, x]] == [bits_of(want_lin)] * 3, (e, lin[y, x])
            assert frame[y, x].tolist() == [want_byte] * 3, (e, frame[y, x])
        exact[e["count"]] += 1
    colours = [f32(e["c_hi"]) for e in grey]
    away = sorted((e["step"], e["count"]) for e in grey if e["distance"] != cs.LADDER_DISTANCES[0])
    print("grey ladder: steps exact on both sides %s of 255 each; colours %.3g .. %.3g; at another distance: %s"
          % (exact, min(colours), max(colours), away))
    assert all(n == 255 for n in exact.values()), exact
    assert min(colours) < 1e-3 and max(colours) > 1.0          # the ladder itself leaves [0, 1]
    assert len(away) <= 4, away


def test_every_stored_coloured_entry_lies_at_three_steps(orc, samples_seeded):
    thr = cs.thresholds(orc)
    coloured = cs.ladder()["coloured"]
    seen = {n: [] for n in cs.LADDER_COUNTS}
    for e in coloured:
        assert len(set(e["steps"])) == 3 and all(hi == lo + 1 for hi, lo in zip(e["rgb_hi"], e["rgb_lo"]))
        for side, offset in (("rgb_hi", 0), ("rgb_lo", 1)):
            rgb = np.array(e[side], np.uint32).view(F)
            frame, lin, _ = cs.ground_render(orc, samples_seeded, rgb, e["count"], e["distance"])
            for ch, (b, (x, y)) in enumerate(zip(e["steps"], e["pixels"])):
                assert bits_of(lin[y, x, ch]) == bits_of(thr[b]) - offset and frame[y, x, ch] == b - offset, (e, side, ch)
            hit = frame[tuple(e["pixels"][0][::-1])]
            assert len(set(hit.tolist())) > 1, "the pixel is not grey"
        seen[e["count"]] += e["steps"]
    print("coloured ladder: %s" % {n: "%d of 255 steps in %d colours" % (len(set(v)), len(v) // 3 * 2) for n, v in seen.items()})
    assert all(sorted(v) == list(range(1, 256)) for v in seen.values())


def test_every_16th_entry_is_what_the_bisection_finds(orc, samples_seeded):
    thr = cs.thresholds(orc)
    n = 0
    for e in cs.ladder()["grey"]:
        if (e["step"] - 1) % 16 == 0 or e["distance"] != cs.LADDER_DISTANCES[0]:
            again, _ = cs.ladder_entry(orc, samples_seeded, thr, e["step"], e["count"])
            assert again == e, (again, e)
            n += 1
    grey = cs.ladder()["grey"]
    assert cs.coloured_of(orc, samples_seeded, grey)[::16] == cs.ladder()["coloured"][::16]
    print("re-derived by bisection: %d grey entries" % n)
    assert n >= 32


def test_the_horizon_tile_has_hits_on_ray_0_alone(orc, samples_seeded):
    h = cs.horizon(orc, samples_seeded)
    thr = cs.thresholds(orc)
    first, second = (h["hits"][:, :, 0] != NO_HIT), (h["hits"][:, :, 1] != NO_HIT)
    print("horizon: distance %g, hits on ray 0: %d, on ray 1: %d; steps %s" % (h["distance"], first.sum(), second.sum(),
                                                                              [e["step"] for e in h["entries"]]))
    assert first.sum() >= 1 and second.sum() == 0
    assert len(h["entries"]) == cs.HORIZON_STEPS and len(h["frames"]) == 2 * cs.HORIZON_STEPS
    for e, (hi, lo) in zip(h["entries"], zip(h["frames"][0::2], h["frames"][1::2])):
        (x, y), b = e["pixel"], e["step"]
        assert first[y, x]
        assert bits_of(hi[3][y, x, 0]) == bits_of(thr[b]) and hi[2][y, x].tolist() == [b] * 3
        assert bits_of(lo[3][y, x, 0]) == bits_of(thr[b]) - 1 and lo[2][y, x].tolist() == [b - 1] * 3


# ---------------------------------------------------------------------------------------------- 2: colour classes
def seen_classes(r, lit):
    """class name -> {"triangle": pixels, "sphere": pixels} whose ray hits the class with at least one lit sample"""
    prims = r["prims"]
    out = {}
    hit = r["hits"] != NO_HIT
    at = np.where(hit, r["hits"], 0)
    some_lit = lit.any(axis=3)
    for c in cs.CLASSES:
        for kind, name in ((0, "triangle"), (1, "sphere")):
            mine = hit & (prims["cls"][at] == c) & (prims["kinds"][at] == kind) & some_lit
            out.setdefault(c, {})[name] = int(mine.any(axis=2).sum())
    return out


def test_every_class_is_seen_lit_on_a_triangle_and_on_a_sphere(orc, samples_seeded):
    r = cs.class_render(orc, samples_seeded, "ordinary", 2, 4)
    assert len(r["prims"]["tris"]) <= 50 and len(r["prims"]["spheres"]) <= 20
    seen = seen_classes(r, cs.lit_table(orc, samples_seeded, "ordinary", 2, 4))
    print("pixels per class: %s" % seen)
    assert all(n >= 1 for kinds in seen.values() for n in kinds.values()), seen


@pytest.mark.parametrize("nb_ray,nb_light", cs.CLASS_CONFIGS)
def test_the_sums_span_the_cases(orc, samples_seeded, nb_ray, nb_light):
    lin = cs.class_render(orc, samples_seeded, "ordinary", nb_ray, nb_light)["lin"]
    with np.errstate(invalid="ignore"):
        n = dict(nan=np.isnan(lin).any(axis=2).sum(), inf=(lin == np.inf).any(axis=2).sum(), negative=(lin < 0).any(axis=2).sum(),
                 above_one=((lin > 1) & np.isfinite(lin)).any(axis=2).sum(), inside=((lin > 0) & (lin < 1)).any(axis=2).sum())
    print("nb_ray %d, %d samples: pixels per kind of sum: %s" % (nb_ray, nb_light, {k: int(v) for k, v in n.items()}))
    assert all(v >= 2 for v in n.values()), n


def tile_kinds(orc, samples, ground, nb_ray, nb_light):
    """per aligned tile: dict of what its hit pixels are, from the oracle"""
    r = cs.class_render(orc, samples, ground, nb_ray, nb_light)
    prims = r["prims"]
    rgb = cs.colour_at(prims)
    out = {}
    for tx, ty, rows, cols in cs.tiles():
        h = r["hits"][rows, cols]
        per_ray = []
        for k in range(nb_ray):
            hit = h[:, :, k] != NO_HIT
            c = rgb[np.where(hit, h[:, :, k], 0)]
            num = np.abs(c[..., 0].astype(np.float64))
            per_ray.append(dict(n_hit=int(hit.sum()), grey=bool(cs.is_grey(c)[hit].all()), any_grey=bool(cs.is_grey(c)[hit].any()),
                                huge=int((hit & (num >= 2.0 ** 61)).sum()), ordinary=int((hit & (num > 0.01) & (num < 1)).sum()),
                                ground_alone=bool((h[:, :, k][hit] == prims["ground"]).all()), hit=hit, colour=c))
        out[(tx, ty)] = per_ray
    return out


def test_the_tiles_are_of_the_kinds_the_layout_says(orc, samples_seeded):
    for nb_ray, nb_light in cs.CLASS_CONFIGS:
        t = tile_kinds(orc, samples_seeded, "ordinary", nb_ray, nb_light)
        grey_with_huge = [k for k, v in t.items() if all(r["grey"] and r["huge"] >= 2 and r["ordinary"] >= 8 for r in v)]
        mixed = [k for k, v in t.items() if all(not r["grey"] and r["any_grey"] for r in v)]
        print("nb_ray %d: grey tiles with a 2^61 member beside ordinary greys %s, mixed tiles %s" % (nb_ray, grey_with_huge, mixed))
        assert (0, 0) in grey_with_huge and (2, 0) in mixed
    # the numerators of the 2^61 grey leave [2^-60, 2^60]: |n.l| of a lit sample on the quad is above one half
    r = cs.class_render(orc, samples_seeded, "ordinary", 1, 4)
    huge = np.isin(r["tri"], np.nonzero(r["prims"]["cls"] == "2^61")[0]) & (np.arange(24)[None, :] < 8)
    assert (r["lin"][huge][:, 0] > 2.0 ** 60).sum() >= 4


def test_a_tile_stops_being_grey_across_rays(orc, samples_seeded):
    for nb_light in (4, 100):
        t = tile_kinds(orc, samples_seeded, "ordinary", 2, nb_light)[(0, 1)]
        r = cs.class_render(orc, samples_seeded, "ordinary", 2, nb_light)
        x, y = cs.SLIVER_PIXEL
        sliver = r["prims"]["sliver"]
        n0, n1 = int((r["hits"][:, :, 0] == sliver).sum()), int((r["hits"][:, :, 1] == sliver).sum())
        print("%d samples: the sliver is met by %d first rays and %d second rays; the tile's second rays: %d hits, grey: %s"
              % (nb_light, n0, n1, t[1]["n_hit"], t[1]["grey"]))
        assert r["hits"][y, x, 0] == sliver and n0 == 1 and n1 == 0
        assert t[1]["grey"] and t[1]["n_hit"] == 64 and not t[0]["grey"]
        assert not cs.is_grey(r["lin"][y, x]), "the pixel's sums must differ: its first ray's samples are lit"


@pytest.mark.parametrize("ground", ["2^61", "+inf"])
def test_an_open_ground_tile_falls_back(orc, samples_seeded, ground):
    for nb_ray, nb_light in cs.CLASS_CONFIGS:
        t = tile_kinds(orc, samples_seeded, ground, nb_ray, nb_light)[(2, 1)]
        assert all(r["n_hit"] == 64 and r["ground_alone"] and r["grey"] for r in t)
        lit = cs.lit_table(orc, samples_seeded, ground, nb_ray, 4)[8:16, 16:24] if nb_light == 4 else None
        assert lit is None or lit.all(), "nothing shadows the open tile"
        lin = cs.class_render(orc, samples_seeded, ground, nb_ray, nb_light)["lin"][8:16, 16:24]
        assert (lin == np.inf).all() if ground == "+inf" else (lin > 2.0 ** 60).all()
    print("ground %s: tile (2, 1) holds 64 ground hits on every ray, every sample lit" % ground)


def test_ladder_values_beside_the_huge_neighbour(orc, samples_seeded):
    thr = cs.thresholds(orc)
    entries = cs.class_ladder(orc, samples_seeded)
    nb_ray, nb_light = cs.CLASS_LADDER_CONFIG
    print("class ladder: steps %s at pixels %s" % ([e["step"] for _, _, e in entries[::2]], sorted({tuple(e["pixel"]) for _, _, e in entries})))
    assert len(entries) == 2 * cs.CLASS_LADDER_STEPS
    for k, (what, rgb, e) in enumerate(entries):
        r = cs.class_render(orc, samples_seeded, "ordinary", nb_ray, nb_light, ladder_rgb=tuple(rgb))
        (x, y), b = e["pixel"], e["step"]
        assert x < 8 and y < 8 and r["tri"][y, x] in r["prims"]["ladder"]
        assert bits_of(r["lin"][y, x, 0]) == bits_of(thr[b]) - k % 2 and r["frame"][y, x].tolist() == [b - k % 2] * 3, what
        assert 0.0 < rgb[0] and cs.is_grey(rgb)


def test_the_whole_stream_scenes_show_the_classes(orc, rtx, samples_seeded):
    for ground in cs.WHOLE_GROUNDS:
        w = cs.whole_stream(orc, rtx, samples_seeded, ground)
        hit = w["tri"] != NO_HIT
        kinds = w["extra"]["kinds"]
        at = np.where(hit, w["tri"], 0)
        rgb = np.zeros((len(kinds), 3), F)
        rgb[kinds == 0], rgb[kinds == 1] = w["rgb"], w["extra"]["sphere_rgb"]
        seen = {bytes(c.tobytes()) for c in rgb[at[hit]]}
        n_ground = int((at[hit] == len(kinds) - 1).sum())
        print("whole stream, ground %s: %d hit pixels, %d on the ground, %d distinct colours seen" % (ground, hit.sum(), n_ground, len(seen)))
        assert len(seen) >= len(cs.CLASSES) and n_ground >= 100 and (kinds[at[hit]] == 1).sum() >= 20
        assert w["stats"]["exact_ties"] == 0 and w["stats"]["nonfinite_t"] == 0
