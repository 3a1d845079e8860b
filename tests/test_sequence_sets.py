"""What the launch sequences of tests/sequence_sets.py can detect, asserted with the oracle alone (no GPU).

tests/test_gpu_sequences.py renders these scenes many times into the library's grow-only buffers and compares each launch
with the oracle's rows.  That only proves something if a launch that did NOT do its work would be seen: its expected bytes
must differ from what the reused output buffer already held, its hit count from every other range's, and the scenes must
put into the workspace what they are there for (queued tiles on P, spheres in the smallest launch of S)."""
import importlib

import numpy as np
import pytest

import gpu_forms as gf
import sequence_sets as sq


@pytest.fixture(scope="module")
def rtx():
    return importlib.import_module("ray-tracer-rust_amd")      # host side only: Wh's mesh generator, scene preparation


@pytest.fixture(scope="module")
def refs(rtx, orc, samples_seeded):
    return {name: sq.reference(name, orc, samples_seeded, rtx) for name in ("P", "S", "G", "B", "Wh")}


def _ranges(ref):
    d = ref["desc"]
    return [(r0, n) for r0, n, _ in sq.launch_sequence(d["H"], d["single"])]


@pytest.mark.parametrize("name", ["P", "S", "G", "B", "Wh"])
def test_every_range_has_hits_of_its_own_and_nothing_needs_a_mask(refs, name):
    ref = refs[name]
    assert ref["nonfinite"] == 0
    ranges = sorted(set(_ranges(ref)))
    hits = {rg: int(ref["hits"][rg[0]:rg[0] + rg[1]].sum()) for rg in ranges}
    print("%s: hits per range %s, rays with a zero component %d (-0.0: %d)"
          % (name, hits, int(ref["zero"].sum()), int(ref["neg_zero"].sum())))
    assert all(h > 0 for h in hits.values()), hits
    for a in ranges:
        for b in ranges:
            if a[1] != b[1]:
                assert hits[a] != hits[b], (a, b, hits[a])
    assert ref["frame"].shape == (ref["desc"]["H"], ref["desc"]["W"], 3)


@pytest.mark.parametrize("name", sq.SEQUENCE_SCENES)
def test_no_launch_of_the_sequence_finds_its_bytes_already_in_the_output_buffer(refs, name):
    """launch k's expected bytes against the leading bytes the buffer held after launch k - 1 (rtx_render_frame's shares
    are launches of their own): a launch that wrote nothing into the reused d_out cannot pass"""
    ref = refs[name]
    H = ref["desc"]["H"]
    launches = [rows for step in sq.full_sequence(H, ref["desc"]["single"]) for rows in sq.step_launches(step, H)]
    assert len(launches) == 8 + 2 + 1
    differs = sq.reused_buffer_differs(ref["frame"], launches)
    assert all(differs), [k + 1 for k, d in enumerate(differs) if not d]


@pytest.mark.parametrize("name", ["P", "S"])
def test_the_packed_shares_of_the_device_resident_launches_differ_from_their_predecessors(refs, name):
    ref = refs[name]
    H = ref["desc"]["H"]
    launches = [sq.share_rows(H, first, stride, sq.ASYNC_TILE_ROWS) for first, stride in sq.async_launches(H)]
    assert sorted(np.concatenate(launches[:3]).tolist()) == list(range(H))          # the three shares are the frame
    assert all(sq.reused_buffer_differs(ref["frame"], launches))
    share_hits = [int(ref["hits"][rows].sum()) for rows in launches]
    print("%s: hits of shares 0, 1, 2, the frame, share 1: %s" % (name, share_hits))
    assert all(h > 0 for h in share_hits) and sum(share_hits[:3]) == share_hits[3]
    # the counter proves ADD only if one share's hits cannot be mistaken for another sum of the launches'
    total = 2 * share_hits[3] + share_hits[1]
    assert total not in (share_hits[1], share_hits[3], share_hits[3] + share_hits[1], 2 * share_hits[3])
    # the first tile number past the frame: the empty share
    assert len(sq.share_rows(H, (H + sq.ASYNC_TILE_ROWS - 1) // sq.ASYNC_TILE_ROWS, sq.ASYNC_SPLIT, sq.ASYNC_TILE_ROWS)) == 0


def test_live_scene_orders_revisit_every_scene_with_other_bytes(refs):
    """per scene, the launches of LIVE_FIRST + LIVE_SECOND in order (each scene has an output buffer of its own; S's is new
    after it was destroyed and created again, and starts with a whole frame's worth of unknown bytes)"""
    assert [n for n, _, _ in sq.LIVE_FIRST] == ["P", "S", "Wh", "G", "S", "P", "Wh", "G"]
    for name in sq.LIVE_SCENES:
        ref = refs[name]
        H = ref["desc"]["H"]
        second = [sq.live_range(H, what) for n, what, _ in sq.LIVE_SECOND if n == name]
        assert len(second) >= 3 and second[-1] == (0, H)
        launches = [np.arange(0, H)] + [np.arange(r0, r0 + n) for r0, n in second]
        assert all(sq.reused_buffer_differs(ref["frame"], launches)), name
        for r0, n in second:
            assert ref["hits"][r0:r0 + n].sum() > 0
    kinds = {(n, c) for n, _, c in sq.LIVE_FIRST + sq.LIVE_SECOND}
    assert kinds == {(n, c) for n in sq.LIVE_SCENES for c in (False, True)}, "every scene runs counted and uncounted"


def test_scene_p_queues_tiles_exactly_in_the_ranges_that_hold_the_centre_row(refs):
    ref = refs["P"]
    d = ref["desc"]
    W, H = d["W"], d["H"]
    assert d["nb_ray"] == 3 and not d["args"][2].any()
    centre = H // 2
    for r0, n in _ranges(ref):
        zero, hard = int(ref["zero"][r0:r0 + n].sum()), int(ref["neg_zero"][r0:r0 + n].sum())
        tiles, _ = sq.launch_tiles(W, n)
        want = sq.tiles_holding_a_hard_ray(ref, r0, n)
        print("P rows (%d, %d): %d rays with a zero component, %d with -0.0, in %d of %d tiles" % (r0, n, zero, hard, want, tiles))
        assert zero >= 3 * n                                   # the centre column crosses every range
        if r0 <= centre < r0 + n:
            assert zero >= 3 * W and hard > 0 and 0 < want <= tiles and not sq.queue_free(ref, r0, n)
        else:
            assert zero == 3 * n and hard == 0 and want == 0 and sq.queue_free(ref, r0, n)
    free = [rg for rg in _ranges(ref) if sq.queue_free(ref, *rg)]
    assert sorted(set(free)) == [(0, 8), (13, 3), (d["single"], 1)]
    # the others: seeded tables, no zero component at all — nothing is ever queued
    for name in ("S", "G", "B", "Wh"):
        assert int(refs[name]["zero"].sum()) == 0, name


def test_scene_s_has_sphere_hits_in_its_smallest_launch(refs, orc):
    ref = refs["S"]
    d = ref["desc"]
    r0, n = d["single"], 1
    assert (r0, n) == min(_ranges(ref), key=lambda rg: rg[1]) == (d["H"] - 1, 1)
    spheres, hits = sq.sphere_hits_in_rows(ref, orc, r0, n)
    print("S rows (%d, %d): %d primary hits, %d on spheres" % (r0, n, hits, spheres))
    assert hits == int(ref["hits"][r0]) and 0 < spheres < hits        # both arms; orc_closest_hit agrees with the render


def test_lds_sizes_and_kernel_forms_differ_between_the_live_scenes(refs, rtx):
    """what alternates through launch_probe's cached grid: three LDS sizes (min(nb_light_sample, 128) samples per batch),
    SPHERES on S only, WHOLE on Wh only"""
    batch = {n: min(refs[n]["desc"]["nb_light"], 128) for n in sq.LIVE_SCENES}
    assert len({batch["P"], batch["S"], batch["G"]}) == 3 and refs["G"]["desc"]["nb_light"] > 128
    assert [n for n in sq.LIVE_SCENES if "spheres" in refs[n]["desc"]["kw"]] == ["S"]
    for name in sq.LIVE_SCENES:
        with sq.make_scene(rtx, refs[name]["desc"]) as s:
            info = s.info()
        assert (info["n_nodes"] > gf.CUT_MAX_NODES) == (name == "Wh"), (name, info["n_nodes"])
        assert info["n_global"] == (1 if name in ("G", "Wh") else 0)
