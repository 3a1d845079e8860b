"""Parity across launch SEQUENCES (run with -m gpu on an MI355X): what survives from one launch to the next.

The other GPU modules create a scene, launch once or twice and destroy it.  Here a scene lives through many launches of
varying size, several scenes live on one device at once, the three families of entry points share one scene's counter
block and events, device-resident renders follow each other without synchronisation, and two host threads call in at once
(include/rtx.h, "Conventions").  The scenes, the orders and the oracle's answers are tests/sequence_sets.py's;
tests/test_sequence_sets.py shows without a GPU that a launch which did not do its work would be seen.  Every comparison
is the project's bar: equal bytes and equal integers."""
import ctypes
import importlib
import threading

import numpy as np
import pytest

import query_sets as qs
import sequence_sets as sq
import shade_sets as ss

pytestmark = pytest.mark.gpu
COUNTS = ("primary_rays", "primary_hits", "shadow_rays", "rays", "box_tests", "tri_tests", "wave_node_visits",
          "wave_tri_visits", "redo_tiles")
RESULT_COUNTS = ("primary_rays", "primary_hits", "shadow_rays", "rays", "redo_tiles")      # what the scene alone decides


@pytest.fixture(scope="module")
def rtx():
    mod = importlib.import_module("ray-tracer-rust_amd")
    assert mod.device_count() >= 1, "no HIP device: the product path has no CPU fallback"
    return mod


@pytest.fixture(scope="module")
def refs(rtx, orc, samples_seeded):
    """name -> sequence_sets.reference: each oracle frame is computed once per process and only sliced afterwards"""
    return lambda name: sq.reference(name, orc, samples_seeded, rtx)


@pytest.fixture(scope="module")
def torch():
    t = pytest.importorskip("torch")
    assert t.cuda.is_available(), "torch sees no GPU"
    return t


def same_rows(img, ref, row0, nrows, what):
    want = ref["frame"][row0:row0 + nrows]
    assert img.shape == want.shape, what
    bad = (img != want).any(axis=2)
    assert not bad.any(), "%s: %d pixels differ from the oracle, first rows %s" % (
        what, int(bad.sum()), sorted(set((np.nonzero(bad)[0] + row0).tolist()))[:8])


def check_counts(st, ref, row0, nrows, what):
    d = ref["desc"]
    hits = int(ref["hits"][row0:row0 + nrows].sum())
    assert st["primary_rays"] == d["nb_ray"] * d["W"] * nrows, what
    assert st["primary_hits"] == hits, (what, st["primary_hits"], hits)
    assert st["shadow_rays"] == d["nb_light"] * hits and st["rays"] == st["primary_rays"] + st["shadow_rays"], what
    tiles, _ = sq.launch_tiles(d["W"], nrows)
    print("%s: redo_tiles %d of %d tiles (tiles holding a -0.0 primary ray: %d)"
          % (what, st["redo_tiles"], tiles, sq.tiles_holding_a_hard_ray(ref, row0, nrows)))
    if sq.queue_free(ref, row0, nrows):
        assert st["redo_tiles"] == 0, (what, st["redo_tiles"])
    else:       # a stale queue entry of a larger predecessor would inflate it
        assert 0 < st["redo_tiles"] <= tiles, (what, st["redo_tiles"], tiles)


def render_and_check(scene, ref, row0, nrows, counted, what):
    if counted:
        img, st = scene.render_rows(row0, nrows, stats=True)
        check_counts(st, ref, row0, nrows, what)
    else:
        img = scene.render_rows(row0, nrows)
    same_rows(img, ref, row0, nrows, what)


# ------------------------------------------------------------------------------------------- 1. one scene, many launches
@pytest.mark.parametrize("name", sq.SEQUENCE_SCENES)
def test_one_scene_through_shrinking_and_growing_launches(rtx, refs, name):
    """launch_sequence with rtx_render_frame's shares in between, all in the buffers the first launch sized: every launch
    is the oracle's rows, every counted one the oracle's hits for its range; on P (nb_ray = 3: running sums in HBM)
    redo_tiles is 0 for the ranges without a -0.0 ray and within the launch's own tile count for the others.  At the end
    the tile descriptors are those of the last launch (where nb_ray = 1 their hit words are the launch's primary hits;
    with more primary rays a descriptor holds one ray's)."""
    ref = refs(name)
    d = ref["desc"]
    W, H = d["W"], d["H"]
    with sq.make_scene(rtx, d) as s:
        for k, step in enumerate(sq.full_sequence(H, d["single"])):
            what = "%s step %d %s" % (name, k, step)
            if step[0] == "rows":
                render_and_check(s, ref, step[1], step[2], step[3], what)
            else:
                same_rows(s.render_frame(step[1], step[2]), ref, 0, H, what)
        td = s.tile_descs(0)
    assert step == ("rows", 0, H, False)
    assert len(td) == sq.launch_tiles(W, H)[1]
    if d["nb_ray"] == 1:
        assert int(td[:, 1].sum()) == int(ref["hits"].sum())


def test_tile_descriptors_shrink_with_the_launch(rtx, refs):
    """the same on a launch SMALLER than its predecessor: descriptors beyond its grid are not reported, the ones inside
    are its own (rows (8, 16) of B — one row of 8 x 8 blocks of tiles — after the whole frame's two)"""
    ref = refs("B")
    d = ref["desc"]
    with sq.make_scene(rtx, d) as s:
        render_and_check(s, ref, 0, d["H"], True, "B whole")
        assert len(s.tile_descs(0)) == sq.launch_tiles(d["W"], d["H"])[1]
        render_and_check(s, ref, 8, 16, False, "B rows (8, 16)")
        td = s.tile_descs(0)
    assert len(td) == sq.launch_tiles(d["W"], 16)[1] < sq.launch_tiles(d["W"], d["H"])[1]
    assert int(td[:, 1].sum()) == int(ref["hits"][8:24].sum())


# ------------------------------------------------------------------------------------------- 2. several live scenes
def test_live_scenes_take_turns_on_one_device(rtx, refs):
    """P, S, G and Wh alive together: SPHERES (S), WHOLE (Wh), COUNT and three LDS sizes alternate through launch_probe's
    per-thread grid cache.  S is destroyed and created again half way."""
    R = {n: refs(n) for n in sq.LIVE_SCENES}
    scenes = {n: sq.make_scene(rtx, R[n]["desc"]) for n in sq.LIVE_SCENES}
    try:
        assert scenes["Wh"].info()["n_nodes"] > sq.gf.CUT_MAX_NODES
        for k, (n, what, counted) in enumerate(sq.LIVE_FIRST):
            r0, nr = sq.live_range(R[n]["desc"]["H"], what)
            render_and_check(scenes[n], R[n], r0, nr, counted, "first order, launch %d: %s (%d, %d)" % (k, n, r0, nr))
        scenes["S"].close()
        scenes["S"] = sq.make_scene(rtx, R["S"]["desc"])
        for k, (n, what, counted) in enumerate(sq.LIVE_SECOND):
            r0, nr = sq.live_range(R[n]["desc"]["H"], what)
            render_and_check(scenes[n], R[n], r0, nr, counted, "second order, launch %d: %s (%d, %d)" % (k, n, r0, nr))
    finally:
        for s in scenes.values():
            s.close()


# ------------------------------------------------------------------------------------------- 3. mixed entry points
@pytest.fixture(scope="module")
def bunny_sets(orc, samples_seeded):
    b = qs.bunny(orc, samples_seeded)
    o, d, exp, _ = b["sets"]["random"]
    _, targets, texp, _ = b["sets"]["random_targets"]
    return dict(trace=(o, d, exp), occlusion=(o, targets, qs.expected_occlusion(texp, o, targets)),
                shade=ss.bunny_sets(orc, samples_seeded)["random"])


def check_trace(got, sets, normals, what):
    qs.check_hits(got, sets["trace"][2], normals, what)


def check_shade(got, sets, what):
    assert got.tobytes() == sets["shade"]["shade"].tobytes(), what + ": shade records differ from the oracle's"


def integers(st, keys=COUNTS):
    return {k: st[k] for k in keys}


def mixed_calls(bunny_sets):
    """the three counted calls of the mixed sequence: name -> call(scene) -> (..., statistics)"""
    o, dirs, _ = bunny_sets["trace"]
    sh = bunny_sets["shade"]
    return {
        "shade": lambda s: s.shade_rays(sh["origins"], sh["directions"], stats=True),
        "render": lambda s: s.render_rows(stats=True),
        "trace": lambda s: s.trace_rays(o, dirs, stats=True, keep_order=True),
    }


def test_render_query_and_shade_take_turns_on_one_scene(rtx, refs, bunny_sets, torch):
    """One counter block and one event pair serve the three families.  Every output is the oracle's, and the fields of
    every RtxStats that the scene alone decides (rays, hits, redo_tiles) are those the same call returns when it is the
    FIRST on a fresh scene (all integer fields, the work counters included: the test below).  Then the header's ordering rule where the families
    cross: a device-resident call with regrouping on a stream of its own, a host call of the OTHER family that uses the
    same sort buffers right behind it, one synchronisation at the end."""
    ref = refs("B")
    d = ref["desc"]
    H = d["H"]
    o, dirs, _ = bunny_sets["trace"]
    oo, targets, occluded = bunny_sets["occlusion"]
    sh = bunny_sets["shade"]
    calls = mixed_calls(bunny_sets)
    fresh = {}
    for key, call in calls.items():
        with sq.make_scene(rtx, d) as s:
            fresh[key] = integers(call(s)[-1], RESULT_COUNTS)
    with sq.make_scene(rtx, d) as s:
        normals = s.normals()
        same_rows(s.render_rows(), ref, 0, H, "render 1")
        check_trace(s.trace_rays(o, dirs, force_regroup=True), bunny_sets, normals, "trace, regrouped")
        got, st = calls["shade"](s)
        check_shade(got, bunny_sets, "shade, counted")
        assert integers(st, RESULT_COUNTS) == fresh["shade"]
        assert np.array_equal(s.occluded_rays(oo, targets), occluded)
        img, st = calls["render"](s)
        same_rows(img, ref, 0, H, "render 2, counted")
        check_counts(st, ref, 0, H, "render 2, counted")
        assert integers(st, RESULT_COUNTS) == fresh["render"]
        got, st = calls["trace"](s)
        check_trace(got, bunny_sets, normals, "trace, counted, caller's order")
        assert integers(st, RESULT_COUNTS) == fresh["trace"]
        assert st["primary_hits"] == int((bunny_sets["trace"][2]["prim"] != qs.NO_HIT).sum()) and st["shadow_rays"] == 0
        got, hits = s.shade_rays(sh["origins"], sh["directions"], force_regroup=True, want_hits=True)
        check_shade(got, bunny_sets, "shade, regrouped, with hits")
        assert np.array_equal(hits["prim"], sh["hit"]["prim"])
        same_rows(s.render_rows(), ref, 0, H, "render 3")

        # shade (device, its own stream) -> trace (host), then trace (device) -> shade (host): no synchronisation between
        stream = torch.cuda.Stream(device="cuda:0")
        n, n_px = len(o), len(sh["origins"])
        t_so, t_sd = torch.from_numpy(sh["origins"]).to("cuda:0"), torch.from_numpy(sh["directions"]).to("cuda:0")
        t_o, t_d = torch.from_numpy(o).to("cuda:0"), torch.from_numpy(dirs).to("cuda:0")
        d_shade = torch.full((n_px * 16,), 0xAA, dtype=torch.uint8, device="cuda:0")
        d_hits = torch.full((n * 32,), 0xAA, dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
        s.shade_rays_device(0, n_px, t_so.data_ptr(), t_sd.data_ptr(), d_shade.data_ptr(), None, stream.cuda_stream,
                            force_regroup=True)
        host_hits = s.trace_rays(o, dirs, force_regroup=True)
        s.trace_rays_device(0, n, t_o.data_ptr(), t_d.data_ptr(), d_hits.data_ptr(), stream.cuda_stream, force_regroup=True)
        host_shade = s.shade_rays(sh["origins"], sh["directions"], force_regroup=True)
        stream.synchronize()
        check_trace(host_hits, bunny_sets, normals, "host trace behind a device-resident shade")
        check_shade(host_shade, bunny_sets, "host shade behind a device-resident trace")
        assert d_shade.cpu().numpy().tobytes() == sh["shade"].tobytes()
        assert d_hits.cpu().numpy().tobytes() == host_hits.tobytes()


def test_statistics_equal_those_of_the_first_call_on_a_fresh_scene(rtx, refs, bunny_sets):
    """Every integer field of every RtxStats of the mixed sequence against the same call made first on a fresh scene:
    the work counters too, which no other test compares between launches.  (This test found them not reproducible for
    rtx_render_rows: with drawn chunks, which wavefront walks a chunk — and so the cut entry its walk begins at — depends
    on timing; box_tests of this frame ranged over 35,638,062 .. 35,671,717 between launches and between fresh scenes,
    the bytes and hits never differed.  The counted cut form now deals its chunks: 35,752,553 every time.)"""
    d = refs("B")["desc"]
    calls = mixed_calls(bunny_sets)
    fresh = {}
    for key, call in calls.items():
        with sq.make_scene(rtx, d) as s:
            fresh[key] = integers(call(s)[-1])
    with sq.make_scene(rtx, d) as s:
        s.render_rows()
        s.trace_rays(*bunny_sets["trace"][:2], force_regroup=True)
        got = {}
        for key in ("shade", "render", "trace"):
            got[key] = integers(calls[key](s)[-1])
            if key == "shade":
                s.occluded_rays(*bunny_sets["occlusion"][:2])
    for key in ("shade", "trace", "render"):
        print(key, "in the sequence", got[key], "first on a fresh scene", fresh[key])
    for key in ("shade", "trace", "render"):
        assert got[key] == fresh[key], key


def test_host_batches_grow_then_shrink_across_the_families(rtx, refs, bunny_sets):
    """The three host entry points share one pair of input buffers and one output buffer, which only grow: a batch of 70
    one-byte answers sizes the output, a shade batch then keeps two segments in it (pixels, and hit records behind them),
    257 regrouped rays follow, the whole occlusion set with statistics, and three pixels at the end.  Every answer is its
    slice of the oracle's (the sets are answered ray by ray; the first 70 pairs hold 17 occluded and 53 lit, the first
    257 rays 138 hits, two of the first three pixels' rays hit); a scene destroyed and created again answers the same."""
    d = refs("B")["desc"]
    o, dirs, exp = bunny_sets["trace"]
    oo, targets, occluded = bunny_sets["occlusion"]
    sh = bunny_sets["shade"]
    n_px = len(sh["shade"])
    assert d["nb_ray"] == 1 and np.array_equal(sh["origins"], o[:n_px]) and np.array_equal(sh["directions"], dirs[:n_px])

    def shade_with_hits(s, what):
        got, hits = s.shade_rays(sh["origins"], sh["directions"], want_hits=True)
        check_shade(got, bunny_sets, what)
        qs.check_hits(hits, exp[:n_px], s.normals(), what)

    with sq.make_scene(rtx, d) as s:
        assert s.occluded_rays(oo[:70], targets[:70]).tobytes() == occluded[:70].tobytes()
        shade_with_hits(s, "shade with hits behind 70 occlusion bytes")
        qs.check_hits(s.trace_rays(o[:257], dirs[:257], force_regroup=True), exp[:257], s.normals(), "257 rays, regrouped")
        got, st = s.occluded_rays(oo, targets, stats=True)
        assert got.tobytes() == occluded.tobytes()
        assert st["primary_rays"] == st["rays"] == len(oo) and st["shadow_rays"] == 0, st
        assert st["primary_hits"] == int(occluded.sum()), (st["primary_hits"], int(occluded.sum()))
        assert s.shade_rays(sh["origins"][:3], sh["directions"][:3]).tobytes() == sh["shade"][:3].tobytes()
    with sq.make_scene(rtx, d) as s:
        shade_with_hits(s, "shade with hits on the scene created again")


# ------------------------------------------------------------------------------------------- 4. back-to-back device renders
def packed(ref, first, stride):
    return ref["frame"][sq.share_rows(ref["desc"]["H"], first, stride, sq.ASYNC_TILE_ROWS)]


def launch_async(torch, scene, ref, stream, counters):
    """the five launches of async_launches into buffers of their own (filler 0xAA), nothing waited for -> the buffers"""
    H = ref["desc"]["H"]
    bufs = []
    for first, stride in sq.async_launches(H):
        nbytes = scene.tiles_bytes(first, stride, sq.ASYNC_TILE_ROWS)
        assert nbytes == len(sq.share_rows(H, first, stride, sq.ASYNC_TILE_ROWS)) * ref["desc"]["W"] * 3
        bufs.append((first, stride, nbytes, torch.full((nbytes + 16,), 0xAA, dtype=torch.uint8, device="cuda:0")))
    stream.wait_stream(torch.cuda.current_stream())          # the fills ran on torch's current stream
    for first, stride, nbytes, buf in bufs:
        scene.render_tiles_device(0, first, stride, sq.ASYNC_TILE_ROWS, buf.data_ptr(), nbytes, stream.cuda_stream,
                                  counters.data_ptr())
    return bufs


def check_async(rtx, ref, bufs, what):
    frame = np.zeros_like(ref["frame"])
    outs = []
    for first, stride, nbytes, buf in bufs:
        out = buf.cpu().numpy()
        assert (out[nbytes:] == 0xAA).all(), what + ": wrote past its share"
        outs.append(out[:nbytes].reshape(-1, ref["desc"]["W"], 3))
        bad = (outs[-1] != packed(ref, first, stride)).any(axis=2)
        assert not bad.any(), "%s: share (%d, %d): %d pixels differ from the oracle" % (what, first, stride, int(bad.sum()))
    for (first, stride, _, _), out in list(zip(bufs, outs))[:3]:
        rtx.scatter_tiles(frame, out, first, stride, sq.ASYNC_TILE_ROWS)
    assert np.array_equal(frame, ref["frame"]), what + ": the three shares do not make the frame"
    assert np.array_equal(outs[3], ref["frame"]) and np.array_equal(outs[4], outs[1]), what


def synchronous_redo(torch, scene, ref):
    """redo_tiles of the same five tile sets, each launched alone into zeroed counters and waited for"""
    total = 0
    for first, stride in sq.async_launches(ref["desc"]["H"]):
        nbytes = scene.tiles_bytes(first, stride, sq.ASYNC_TILE_ROWS)
        buf = torch.zeros(nbytes, dtype=torch.uint8, device="cuda:0")
        ctr = torch.zeros(8, dtype=torch.int64, device="cuda:0")
        torch.cuda.synchronize()
        scene.render_tiles_device(0, first, stride, sq.ASYNC_TILE_ROWS, buf.data_ptr(), nbytes,
                                  torch.cuda.current_stream().cuda_stream, ctr.data_ptr())
        torch.cuda.synchronize()
        total += int(ctr[5])
    return total


def expected_hits(ref):
    share1 = int(ref["hits"][sq.share_rows(ref["desc"]["H"], 1, sq.ASYNC_SPLIT, sq.ASYNC_TILE_ROWS)].sum())
    return 2 * int(ref["hits"].sum()) + share1


@pytest.mark.parametrize("name", ["P", "S"])
def test_device_resident_renders_back_to_back(rtx, refs, torch, name):
    """As bench.py launches: no synchronisation between launches of different sizes that share the workspace, first on
    torch's current stream, then (the buffers now at their full size: nothing is reallocated in between) on a fresh one.
    The kernels ADD into the caller's counters: word 0 ends at twice the frame's hits plus share 1's, word 5 at the sum of
    what the same launches count one at a time."""
    ref = refs(name)
    with sq.make_scene(rtx, ref["desc"]) as s:
        for which in ("current", "fresh"):
            stream = torch.cuda.current_stream() if which == "current" else torch.cuda.Stream(device="cuda:0")
            counters = torch.zeros(8, dtype=torch.int64, device="cuda:0")
            bufs = launch_async(torch, s, ref, stream, counters)
            stream.synchronize()
            torch.cuda.synchronize()
            check_async(rtx, ref, bufs, "%s on the %s stream" % (name, which))
            got = counters.cpu().numpy()
            assert int(got[0]) == expected_hits(ref), (which, got)
            redo = synchronous_redo(torch, s, ref)
            print("%s, %s stream: counters %s, redo_tiles one at a time %d" % (name, which, got.tolist(), redo))
            assert int(got[5]) == redo, (which, got, redo)
            assert (redo > 0) == (name == "P")


def test_two_scenes_alternate_on_one_stream_without_synchronisation(rtx, refs, torch):
    R = {n: refs(n) for n in ("P", "S")}
    scenes = {n: sq.make_scene(rtx, R[n]["desc"]) for n in R}
    try:
        stream = torch.cuda.Stream(device="cuda:0")
        counters = {n: torch.zeros(8, dtype=torch.int64, device="cuda:0") for n in R}
        plan = {n: [] for n in R}
        for n in R:
            for first, stride in sq.async_launches(R[n]["desc"]["H"]):
                nbytes = scenes[n].tiles_bytes(first, stride, sq.ASYNC_TILE_ROWS)
                plan[n].append((first, stride, nbytes, torch.full((nbytes + 16,), 0xAA, dtype=torch.uint8, device="cuda:0")))
            scenes[n].upload(0)
        stream.wait_stream(torch.cuda.current_stream())
        for k in range(5):
            for n in ("P", "S"):
                first, stride, nbytes, buf = plan[n][k]
                scenes[n].render_tiles_device(0, first, stride, sq.ASYNC_TILE_ROWS, buf.data_ptr(), nbytes, stream.cuda_stream,
                                              counters[n].data_ptr())
        stream.synchronize()
        for n in R:
            check_async(rtx, R[n], plan[n], n + ", alternating")
            assert int(counters[n][0]) == expected_hits(R[n]), n
    finally:
        for s in scenes.values():
            s.close()


def test_the_empty_share_writes_nothing(rtx, refs, torch):
    """first_tile = the number of row tiles: no rows, RTX_OK with a valid pointer and d_out_bytes = 0; nothing is written,
    the counters keep their values, and the launches around it are unharmed"""
    ref = refs("S")
    H = ref["desc"]["H"]
    n_tiles = (H + sq.ASYNC_TILE_ROWS - 1) // sq.ASYNC_TILE_ROWS
    stream = torch.cuda.current_stream().cuda_stream
    with sq.make_scene(rtx, ref["desc"]) as s:
        assert s.tiles_rows(n_tiles, sq.ASYNC_SPLIT, sq.ASYNC_TILE_ROWS) == 0
        assert s.tiles_bytes(n_tiles, sq.ASYNC_SPLIT, sq.ASYNC_TILE_ROWS) == 0
        assert s.tiles_rows(n_tiles - 1, sq.ASYNC_SPLIT, sq.ASYNC_TILE_ROWS) == H - (n_tiles - 1) * sq.ASYNC_TILE_ROWS > 0
        guard = torch.full((16,), 0xAA, dtype=torch.uint8, device="cuda:0")
        counters = torch.arange(1, 9, dtype=torch.int64, device="cuda:0")
        for before in (False, True):        # on a scene that has not launched yet, and between two launches
            if before:
                same_rows(s.render_rows(), ref, 0, H, "before the empty share")
            rc = rtx.rtx._lib.rtx_render_tiles_device(s.handle, 0, n_tiles, sq.ASYNC_SPLIT, sq.ASYNC_TILE_ROWS,
                                                      ctypes.c_void_p(guard.data_ptr()), 0, ctypes.c_void_p(stream),
                                                      ctypes.c_void_p(counters.data_ptr()))
            assert rc == rtx.OK
            torch.cuda.synchronize()
            assert (guard.cpu().numpy() == 0xAA).all()
            assert counters.cpu().numpy().tolist() == list(range(1, 9))
        render_and_check(s, ref, 0, H, True, "after the empty share")


# ------------------------------------------------------------------------------------------- 5. host threads
class Caller(threading.Thread):
    """a daemon thread that runs `work(self)`; self.at names the call it is in (ctypes releases the GIL inside it)"""

    def __init__(self, name, work):
        super().__init__(name=name, daemon=True)
        self.work, self.at, self.error = work, "not started", None

    def run(self):
        try:
            self.work(self)
            self.at = "done"
        except BaseException as e:      # reported by the test's thread
            self.error = e


def run_together(scenes, *callers):
    for c in callers:
        c.start()
    for c in callers:
        c.join(timeout=60)
    stuck = [c for c in callers if c.is_alive()]
    if stuck:
        for s in scenes:                # start nothing more on the device: the handles are left alone, not destroyed
            s._h = ctypes.c_void_p()
        pytest.fail("still running after 60 s: " + "; ".join("%s in %s" % (c.name, c.at) for c in stuck))
    for c in callers:
        if c.error is not None:
            raise c.error


def test_two_threads_render_disjoint_rows_of_one_scene(rtx, refs):
    """(a) same scene, same device: the calls are serialised inside the library"""
    ref = refs("B")
    H = ref["desc"]["H"]
    halves = {"upper": (0, 61), "lower": (61, H - 61)}
    got = {k: [] for k in halves}
    with sq.make_scene(rtx, ref["desc"]) as s:
        def work(me):
            r0, n = halves[me.name]
            for k in range(4):
                me.at = "render_rows(%d, %d) number %d" % (r0, n, k)
                got[me.name].append(s.render_rows(r0, n))
        run_together([s], *[Caller(k, work) for k in halves])
    for k, (r0, n) in halves.items():
        assert len(got[k]) == 4
        for j, img in enumerate(got[k]):
            same_rows(img, ref, r0, n, "%s thread, render %d" % (k, j))


def test_two_threads_render_a_scene_each(rtx, refs):
    """(b) P and S, one thread each: two library streams on one device at once, each grid sized to fill it; counted and
    uncounted launches alternate (each thread has launch_probe's cache of its own)"""
    R = {n: refs(n) for n in ("P", "S")}
    scenes = {n: sq.make_scene(rtx, R[n]["desc"]) for n in R}
    got = {n: [] for n in R}
    try:
        def work(me):
            for k in range(4):
                me.at = "render_rows(stats=%s) number %d on scene %s" % (bool(k & 1), k, me.name)
                got[me.name].append(scenes[me.name].render_rows(stats=True) if k & 1 else (scenes[me.name].render_rows(), None))
        run_together(list(scenes.values()), *[Caller(n, work) for n in R])
    finally:
        for s in scenes.values():
            s.close()
    for n in R:
        assert len(got[n]) == 4
        for j, (img, st) in enumerate(got[n]):
            same_rows(img, R[n], 0, R[n]["desc"]["H"], "%s render %d" % (n, j))
            if st is not None:
                check_counts(st, R[n], 0, R[n]["desc"]["H"], "%s render %d" % (n, j))


def test_one_thread_renders_while_the_other_queries_and_shades(rtx, refs, bunny_sets):
    """(c) one scene: render_rows against trace_rays / shade_rays, which share its counter block, events and stream"""
    ref = refs("B")
    H = ref["desc"]["H"]
    o, dirs, _ = bunny_sets["trace"]
    sh = bunny_sets["shade"]
    frames, traced, shaded = [], [], []
    with sq.make_scene(rtx, ref["desc"]) as s:
        normals = s.normals()

        def render(me):
            for k in range(4):
                me.at = "render_rows(stats=%s) number %d" % (bool(k & 1), k)
                frames.append(s.render_rows(stats=True) if k & 1 else (s.render_rows(), None))

        def query(me):
            for k in range(2):
                me.at = "trace_rays number %d" % k
                traced.append(s.trace_rays(o, dirs, stats=bool(k), force_regroup=not k))
                me.at = "shade_rays number %d" % k
                shaded.append(s.shade_rays(sh["origins"], sh["directions"], stats=bool(k), force_regroup=not k))
        run_together([s], Caller("render", render), Caller("query", query))
    assert len(frames) == 4 and len(traced) == len(shaded) == 2
    for j, (img, st) in enumerate(frames):
        same_rows(img, ref, 0, H, "render %d beside queries" % j)
        if st is not None:
            check_counts(st, ref, 0, H, "render %d beside queries" % j)
    n_hits = int((bunny_sets["trace"][2]["prim"] != qs.NO_HIT).sum())
    check_trace(traced[0], bunny_sets, normals, "trace beside renders")
    check_trace(traced[1][0], bunny_sets, normals, "counted trace beside renders")
    assert traced[1][1]["primary_hits"] == n_hits and traced[1][1]["shadow_rays"] == 0
    check_shade(shaded[0], bunny_sets, "shade beside renders")
    check_shade(shaded[1][0], bunny_sets, "counted shade beside renders")
    shade_hits = int((sh["hit"]["prim"] != qs.NO_HIT).sum())
    assert shaded[1][1]["primary_hits"] == shade_hits and shaded[1][1]["shadow_rays"] == ref["desc"]["nb_light"] * shade_hits
