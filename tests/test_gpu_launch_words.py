"""The words a render launch counts in (run with -m gpu on an MI355X).

A launch of the two-pass pipeline is four dispatches — probe_kernel, order_tiles_kernel, shade_tiles_kernel,
reference_tiles_kernel (the whole-stream form keeps count_classes_kernel as a fifth) — and none of them only zeroes: the
queue's counts, the histogram of cost classes, the order's cursors and the claim words are zeroed for the NEXT pass or
the NEXT launch by a kernel the launch runs anyway, selected by the parity of how many launches and passes the workspace
has served, and zeroed by reset_kernel once when a buffer is allocated or grown (csrc/rtx_pass_order.hpp, the table at
order_tiles_kernel; csrc/rtx_api.cpp, render_launch).  A workgroup's first job
is dealt by its number and only the later ones are claimed.  A word left stale shows as a wrong byte, a wrong
primary_hits / redo_tiles, a tile rendered twice or not at all; so every launch here is compared, with zero tolerance,
with rtx_render_view of the same rows (its kernels use none of these words) and with the same launch made earlier, and
the sequences are of odd and even length so that every kind of launch meets both parities.

order_tiles_kernel also picks the share of the split limit from which a cost class runs raised by the launch's size: an
eighth below kRaisedSmallJobs = 64 scheduled tiles per workgroup, a quarter from there (the jobs' levels).  The last two
tests make launches on either side of that size on one workspace, so that the raised end of the order — the word every
pass rewrites — moves between the whole order, a part of it and zero."""
import importlib
import json
import os

import numpy as np
import pytest

import gpu_forms as gf
import sequence_sets as sq

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUNNY = os.path.join(ROOT, "models", "big_bunny.obj")
GOLDEN = os.path.join(ROOT, "tests", "golden")
COUNTS = ("primary_rays", "primary_hits", "shadow_rays", "rays", "box_tests", "tri_tests", "wave_node_visits",
          "wave_tri_visits", "redo_tiles")
VIEW_COUNTS = ("primary_rays", "primary_hits", "shadow_rays", "rays")     # what the scene alone decides


@pytest.fixture(scope="module")
def rtx():
    mod = importlib.import_module("ray-tracer-rust_amd")
    assert mod.device_count() >= 1, "no HIP device: the product path has no CPU fallback"
    return mod


class Checked:
    """One scene: every launch against rtx_render_view of its rows (rendered once per range) and against the first
    launch of the same range."""

    def __init__(self, scene, what):
        self.scene, self.what, self.views, self.first, self.launches = scene, what, {}, {}, 0

    def view(self, row0, nrows):
        if (row0, nrows) not in self.views:
            v = self.scene.own_view()
            v.x0, v.y0, v.nx, v.ny = 0, row0, v.width, nrows
            img, st = self.scene.render_view(v, stats=True)
            img.setflags(write=False)
            self.views[(row0, nrows)] = (img, st)
        return self.views[(row0, nrows)]

    def same(self, img, want, what):
        assert img.shape == want.shape, what
        bad = (img != want).any(axis=2)
        ys, xs = np.nonzero(bad)
        assert not bad.any(), "%s: %d pixels differ; first (x, y): %s" % (what, int(bad.sum()), list(zip(xs[:8].tolist(), ys[:8].tolist())))

    def rows(self, row0, nrows, counted):
        """one launch -> its statistics (counted) or None"""
        self.launches += 1
        what = "%s, launch %d: rows (%d, %d)%s" % (self.what, self.launches, row0, nrows, " counted" if counted else "")
        want, vst = self.view(row0, nrows)
        if not counted:
            self.same(self.scene.render_rows(row0, nrows), want, what)
            return None
        img, st = self.scene.render_rows(row0, nrows, stats=True)
        self.same(img, want, what)
        ints = {k: int(st[k]) for k in COUNTS}
        print(what, ints)
        for k in VIEW_COUNTS:
            assert ints[k] == int(vst[k]), (what, k, ints[k], int(vst[k]))
        assert ints == self.first.setdefault((row0, nrows), ints), (what, ints, self.first[(row0, nrows)])
        return ints


# ------------------------------------------------------------------------------------------------------ sequences
def test_queued_and_queue_free_launches_alternate(rtx, orc, samples_seeded):
    """Scene P (nb_ray = 3, -0.0 primary rays in row 20): launches that queue tiles for the reference re-render alternate
    with launches that queue none, counted and uncounted, thirteen launches: each kind of launch works on each of the two
    queues at least twice.  A count left from the launch before shows in redo_tiles and primary_hits."""
    d = sq.description("P", orc, samples_seeded)
    H = d["H"]
    with sq.make_scene(rtx, d) as s:
        c = Checked(s, "P")
        queued, free = [], []
        for row0, nrows, counted in [(0, H, True), (0, 8, True), (0, H, True), (13, 3, True), (5, H - 5, True), (0, 8, False),
                                     (0, 8, True), (0, H, True), (5, H - 5, True), (0, 8, True), (0, H, True), (0, H, True),
                                     (13, 3, True)]:
            st = c.rows(row0, nrows, counted)
            if st is not None:
                (queued if row0 + nrows > 20 >= row0 else free).append((c.launches & 1, st["redo_tiles"]))
    print("queued", queued, "free", free)
    assert all(n > 0 for _, n in queued) and all(n == 0 for _, n in free)
    for kind in (queued, free):
        assert sum(1 for p, _ in kind if p == 0) >= 2 and sum(1 for p, _ in kind if p == 1) >= 2


# ------------------------------------------------------------------------------- shrinking work, shares, workspace growth
@pytest.fixture(scope="module")
def ragged_golden():
    from PIL import Image
    with open(os.path.join(GOLDEN, "golden.json")) as f:
        case = json.load(f)["cases"]["ragged_bigbunny_203x117_seed"]
    img = np.asarray(Image.open(os.path.join(GOLDEN, "ragged_bigbunny_203x117_seed.png")).convert("RGB"))
    return case, img


def test_many_rows_then_few_then_shares(rtx, samples_seeded, ragged_golden):
    """big_bunny at 203 x 117 (fewer jobs than workgroups): the whole frame, then few rows, one row, the strided shares of
    rtx_render_frame and the whole frame again, all in the first launch's workspace: list entries, counts and claims of
    the larger launch are still in memory behind the smaller one's."""
    case, golden = ragged_golden
    W, H = 203, 117
    with rtx.default_scene([BUNNY], W, H, samples_seeded) as s:
        c = Checked(s, "B")
        st = c.rows(0, H, True)
        assert st["primary_hits"] == case["primary_hits"]
        c.same(s.render_rows(), golden, "B against the golden")
        for row0, nrows, counted in [(8, 16, True), (H - 1, 1, True), (0, H, True), (8, 16, False), (8, 16, True), (40, 9, True)]:
            c.rows(row0, nrows, counted)
        for devices, tile_rows in [((0, 0), 5), ((0, 0, 0), 8), ((0,), 16)]:      # shares (first_tile, stride) of one device
            c.same(s.render_frame(devices, tile_rows), golden, "B render_frame %s %d" % (devices, tile_rows))
            c.rows(40, 9, True)
        c.rows(0, H, True)


def test_workspace_grows_and_is_used_small_again(rtx, samples_seeded):
    """A small launch allocates, a larger one grows the workspace and the queue (their counting words are zeroed then), the small one
    follows in the grown buffers; twice, so that the growth falls on either parity of the small launches before it."""
    W, H = 203, 117
    for before in (1, 2):
        with rtx.default_scene([BUNNY], W, H, samples_seeded) as s:
            c = Checked(s, "grow after %d" % before)
            for _ in range(before):
                c.rows(16, 8, True)
            c.rows(0, 64, True)
            c.rows(16, 8, True)
            c.rows(0, H, True)
            c.rows(16, 8, True)
            c.rows(0, 64, True)


# ------------------------------------------------------------------------------------------------------ nb_ray = 2
def test_two_primary_rays_keep_the_queue_and_refresh_the_order(rtx, samples_seeded):
    """nb_ray = 2: the second pass of a launch has a fresh histogram, fresh cursors and claims and the first pass's queue.
    big_bunny at 64 x 48, five launches, whole frames and a range."""
    tris, rgb = rtx.default_primitives([BUNNY])
    with rtx.Scene(64, 48, tris, rgb, samples_seeded, nb_ray=2) as s:
        c = Checked(s, "bunny nb_ray 2")
        for row0, nrows, counted in [(0, 48, True), (0, 48, False), (0, 48, True), (16, 24, True), (0, 48, True)]:
            st = c.rows(row0, nrows, counted)
        assert st["primary_rays"] == 2 * 64 * 48 and st["primary_hits"] > 0


# ------------------------------------------------------------------------------- fewer jobs than workgroups, more than the grid
@pytest.mark.parametrize("W,H", [(8, 8), (24, 16), (203, 117)])
def test_fewer_jobs_than_workgroups(rtx, samples_seeded, W, H):
    """one tile, six tiles, 390 tiles: most workgroups are dealt nothing and leave; the centre crop of the default frame"""
    with rtx.default_scene([BUNNY], W, H, samples_seeded) as s:
        c = Checked(s, "%d x %d" % (W, H))
        for counted in (True, False, True, True):
            st = c.rows(0, H, counted)
        assert st["primary_hits"] > 0


def test_more_jobs_than_the_grid_each_tile_rendered_once(rtx, samples_seeded):
    """The ground alone, seen from above at 512 x 304: 64 x 38 = 2,432 tiles, every pixel a hit, one cost class: the first
    1,024 jobs are dealt and the rest claimed.  Every tile's bytes land in a buffer filled with another value, the tile
    descriptors hold every hit once, and a second and third launch say the same."""
    torch = pytest.importorskip("torch")
    W, H = 512, 304
    tris = np.asarray(rtx.GROUND_TRI, np.float32).reshape(1, 9)
    rgb = np.full((1, 3), 0.5, np.float32)
    with rtx.Scene(W, H, tris, rgb, samples_seeded, look_at=(0.0, 0.0, 100.0), nb_light_sample=16) as s:
        c = Checked(s, "ground")
        want, vst = c.view(0, H)
        assert int(vst["primary_hits"]) == W * H
        for k in range(3):
            st = c.rows(0, H, True)
            assert st["primary_hits"] == W * H and st["redo_tiles"] == 0
            td = s.tile_descs(0)
            assert int((td[:, 1] == 64).sum()) == (W // 8) * (H // 8) and int(td[:, 1].sum()) == W * H
            buf = torch.full((H * W * 3,), 0x5A + k, dtype=torch.uint8, device="cuda:0")
            s.render_tiles_device(0, 0, 1, H, buf.data_ptr(), buf.numel(), torch.cuda.current_stream().cuda_stream, None)
            torch.cuda.synchronize()
            c.same(buf.cpu().numpy().reshape(H, W, 3), want, "ground, device-resident launch %d" % k)


# ------------------------------------------------------------------------------------------------------ split tiles
def test_a_share_whose_tiles_are_split_into_parts(rtx, samples_seeded):
    """tests/test_gpu_job_priority.py's sets: big_bunny at 512 x 384 (3,072 tiles, mixed classes, three times the grid) and
    its share (3, 8, 8) — 384 tiles for 1,024 workgroups, so the costly tiles are cut into parts and the parts are dealt."""
    torch = pytest.importorskip("torch")
    W, H = 512, 384
    first, stride, rows = 3, 8, 8
    with rtx.default_scene([BUNNY], W, H, samples_seeded) as s:
        c = Checked(s, "512 x 384")
        whole, _ = c.view(0, H)
        want = np.concatenate([whole[t * rows:(t + 1) * rows] for t in range(first, (H + rows - 1) // rows, stride)])
        nbytes = s.tiles_bytes(first, stride, rows)
        for k in range(3):
            c.rows(0, H, k != 1)
            buf = torch.full((nbytes,), 0x5A, dtype=torch.uint8, device="cuda:0")
            s.render_tiles_device(0, first, stride, rows, buf.data_ptr(), nbytes, torch.cuda.current_stream().cuda_stream, None)
            torch.cuda.synchronize()
            c.same(buf.cpu().numpy().reshape(-1, W, 3), want, "share (3, 8, 8), time %d" % k)
            if k == 1:
                c.rows(24, 8, True)


# ------------------------------------------------------------------------------------------------------ whole-stream form
def test_whole_stream_form(rtx, samples_seeded):
    """sequence_sets' scene Wh (more stream records than a tile's cut may refer to: jobs are claimed per XCD group, none is
    dealt): shrinking and growing launches, five and more, counted and not."""
    tris, rgb, extra = gf.whole_stream_scene(rtx)
    assert not extra
    with rtx.Scene(24, 24, tris, rgb, samples_seeded, nb_ray=1, nb_light_sample=4, leaf_max=1,
                   reference_tree=rtx.REFTREE_NEVER, tie_rank=None) as s:
        assert s.info()["n_nodes"] > gf.CUT_MAX_NODES
        c = Checked(s, "Wh")
        for row0, nrows, counted in [(0, 24, True), (0, 8, True), (0, 24, False), (13, 3, True), (0, 24, True), (0, 8, True),
                                     (13, 3, True)]:
            st = c.rows(row0, nrows, counted)
        assert st["primary_hits"] > 0


# ------------------------------------------------------------------------------------------------------ both raised shares
GRID = 1024                      # resident workgroups of shade_tiles_kernel on an MI355X: 256 CUs x 4
RAISED_SMALL_JOBS = 64           # rtx_pass_order.hpp, kRaisedSmallJobs
TILE_UNSCHEDULED = 0xFFFFFFFF    # a descriptor's cost class when the tile has no job (no hit, or queued)


def scheduled_per_workgroup(scene):
    """tiles of the most recent launch that order_tiles_kernel scheduled, per workgroup of the grid"""
    td = scene.tile_descs(0)
    return int((td[:, 0] != TILE_UNSCHEDULED).sum()) / GRID


def either_side_of_the_raised_rule(c, H, small, middle):
    """whole frame (a quarter), a few rows (an eighth), whole, a middle range, few, whole, few: seven launches, the large
    one on both parities, every one against rtx_render_view and against its first time; -> per_wg of each kind"""
    per_wg = {}
    for (row0, nrows), counted in [((0, H), True), (small, True), ((0, H), True), (middle, True), (small, False),
                                   (small, True), ((0, H), True)]:
        c.rows(row0, nrows, counted)
        per_wg.setdefault((row0, nrows), scheduled_per_workgroup(c.scene))
    print(c.what, "scheduled tiles per workgroup:", per_wg)
    return per_wg


def test_raised_share_rule_both_values_ground_only(rtx, samples_seeded):
    """The ground alone at 2304 x 2048: 73,728 tiles of one cost class, 72 per workgroup — the quarter branch, and an
    order_tiles_kernel of 72 workgroups zeroing the next pass's set (more workgroups than the set has thousands of words).
    One class at a fair share of 72 tiles is far from a quarter of the limit: the raised end is ZERO there, and the WHOLE
    order in the launches of a few rows between them (under one job per workgroup, the limit is a fraction of a tile)."""
    W, H = 2304, 2048
    tris = np.asarray(rtx.GROUND_TRI, np.float32).reshape(1, 9)
    rgb = np.full((1, 3), 0.5, np.float32)
    # (looking down at 45 degrees from a distance of 2000 pixels: the frame's half height is 27 degrees, every ray goes down)
    with rtx.Scene(W, H, tris, rgb, samples_seeded, look_at=(0.0, 0.0, 100.0), distance=2000.0, nb_light_sample=4) as s:
        c = Checked(s, "ground 2304 x 2048")
        per_wg = either_side_of_the_raised_rule(c, H, (1024, 8), (512, 560))
        assert c.first[(0, H)]["primary_hits"] == W * H
    assert per_wg[(0, H)] >= RAISED_SMALL_JOBS > per_wg[(512, 560)] > per_wg[(1024, 8)] > 0


def test_raised_share_rule_both_values_mixed_classes(rtx, samples_seeded):
    """big_bunny at 3328 x 3072 (159,744 tiles, the upper part sky): classes from open ground to the mesh's silhouette, so
    the raised end is a PART of the order on either side of the rule — at a quarter in the whole frame, at an eighth in
    the ranges through the bunny — and the three launch sizes leave three different ends in the one word."""
    W, H = 3328, 3072
    with rtx.default_scene([BUNNY], W, H, samples_seeded, nb_light_sample=8) as s:
        c = Checked(s, "big_bunny 3328 x 3072")
        per_wg = either_side_of_the_raised_rule(c, H, (1536, 24), (1300, 600))
        assert c.first[(1536, 24)]["primary_hits"] > 0
    assert per_wg[(0, H)] >= RAISED_SMALL_JOBS > per_wg[(1300, 600)] > per_wg[(1536, 24)] > 0
