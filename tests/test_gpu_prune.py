"""GPU parity of the closest-hit walks where pruning by distance could change the answer: rays whose oracle hit is a
triangle BEHIND a wall with a computed distance IN FRONT of it (tests/prune_sets.py; the fixtures' conditions, and the
emulation that calls these rays exposed, are stated without a GPU by tests/test_prune_sets.py).  The reference takes the
minimum of the computed distances over every candidate, so a walk that leaves a box out because it is entered beyond
the closest hit so far answers such a ray with the wall.  rtx_trace_rays, rtx_occluded_rays (the any-hit walk: the control
that the scenes themselves are handled), rtx_shade_rays and the 1 x 1 frames of the three render entry points, with and
without statistics, on a scene of triangles and on one holding a sphere, each in two stream orders.  No tolerance."""
import importlib

import numpy as np
import pytest

import gpu_forms
import prune_sets as ps
import query_sets as qs
from test_gpu_shade_rays import shade_every_way
from test_gpu_trace_rays import occluded_every_way, trace_every_way

pytestmark = pytest.mark.gpu
NAMES = ("triangles", "sphere")
CASES = [(n, o) for n in NAMES for o in ps.ORDERS]


@pytest.fixture(scope="module")
def rtx():
    mod = importlib.import_module("ray-tracer-rust_amd")
    assert mod.device_count() >= 1, "no HIP device: the product path has no CPU fallback"
    assert mod.rtx.RAY_HIT_DTYPE == qs.HIT_DTYPE
    return mod


@pytest.fixture(scope="module")
def scenes(rtx, orc, samples_seeded):
    """(name, order) -> dict(b = prune_sets.Built, scene = the library's scene of the same arguments, sets, normals)"""
    made = {}

    def get(name, order):
        if (name, order) not in made:
            b = ps.scene(rtx, orc, samples_seeded, name)[order]
            scene = rtx.Scene(*b.args, **b.kw)
            assert scene.info()["n_global"] == 0 and scene.info()["n_ref_nodes"] != 0
            made[name, order] = dict(b=b, scene=scene, sets=ps.ray_sets(rtx, orc, samples_seeded, name)[order], stored=scene.normals())
        return made[name, order]
    yield get
    for m in made.values():
        m["scene"].close()


def trace(m, ray_set, what, every_way=True):
    o, d, exp, _ = ray_set
    if every_way:
        got = trace_every_way(m["scene"], o, d, exp, None, what)
    else:
        got = m["scene"].trace_rays(o, d, keep_order=True)
        qs.check_hits(got, exp, None, what)
    qs.check_normals(got, exp, m["stored"], m["b"].kinds, what)
    return got


# ---------------------------------------------------------------------------------------------- rtx_trace_rays
@pytest.mark.parametrize("name,order", CASES)
def test_a_single_rays(scenes, name, order):
    """one ray to a batch: the wavefront's only voting lane"""
    m = scenes(name, order)
    o, d, exp, _ = m["sets"]["exposed"]
    for k in (0, 1, 63, 64, 127):
        trace(m, (o[k:k + 1], d[k:k + 1], exp[k:k + 1], None), "%s %s ray %d alone" % (name, order, k), every_way=False)


@pytest.mark.parametrize("n", [64, 128])
@pytest.mark.parametrize("name,order", CASES)
def test_b_whole_wavefronts_of_exposed_rays(scenes, name, order, n):
    """64 and 128 rays of one ill-conditioned triangle from the start of the batch: in the caller's order every lane of a
    wavefront agrees that the box behind the wall lies beyond its closest hit"""
    m = scenes(name, order)
    o, d, exp, _ = m["sets"]["exposed"]
    assert (exp["prim"][:n] == m["b"].groups["behind"][0]).all()
    trace(m, (o[:n], d[:n], exp[:n], None), "%s %s %d exposed rays" % (name, order, n))


@pytest.mark.parametrize("name,order", CASES)
def test_c_exposed_rays_among_ordinary_ones(scenes, name, order):
    """the same rays shuffled among 1,000 ordinary ones: caller's order, default flags, regrouping forced"""
    m = scenes(name, order)
    trace(m, m["sets"]["mixed"], "%s %s mixed" % (name, order))


@pytest.mark.parametrize("name,order", CASES)
def test_d_controls(scenes, name, order):
    """triangles in front of the wall whose distance comes out behind it, well-conditioned triangles and a sphere behind it"""
    m = scenes(name, order)
    for key in ("front", "well") + (("sphere",) if name == "sphere" else ()):
        trace(m, m["sets"][key], "%s %s %s" % (name, order, key))


def test_device_resident_trace(rtx, scenes):
    torch = pytest.importorskip("torch")
    assert torch.cuda.is_available(), "torch sees no GPU"
    m = scenes("triangles", "built")
    o, d, exp, _ = m["sets"]["exposed"]
    n = len(o)
    t_o, t_d = torch.from_numpy(o).to("cuda:0"), torch.from_numpy(d).to("cuda:0")
    hits = torch.full((n * 32,), 0xAA, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    m["scene"].trace_rays_device(0, n, t_o.data_ptr(), t_d.data_ptr(), hits.data_ptr(), None, keep_order=True)
    torch.cuda.synchronize()
    got = hits.cpu().numpy().view(rtx.rtx.RAY_HIT_DTYPE)
    qs.check_hits(got, exp, None, "device-resident, 128 exposed rays")


# ---------------------------------------------------------------------------------------------- rtx_occluded_rays
@pytest.mark.parametrize("name,order", CASES)
def test_occlusion_on_the_same_rays(orc, scenes, name, order):
    """the any-hit walk has no pruning: targets beyond the wall along the same rays"""
    m = scenes(name, order)
    for key in ("exposed", "mixed"):
        o, d, _, _ = m["sets"][key]
        oo, t, _, want = ps.occlusion_set(orc, m["b"], o, d)
        if key == "exposed":
            assert want.all()
        occluded_every_way(m["scene"], oo, t, want, "%s %s %s" % (name, order, key))


# ---------------------------------------------------------------------------------------------- rtx_shade_rays
@pytest.mark.parametrize("name,order", CASES)
def test_shading_whole_wavefronts_of_exposed_rays(orc, samples_seeded, scenes, name, order):
    """linear colour bit for bit, RGB8, and the hit records rtx_trace_rays writes (shade_every_way)"""
    m = scenes(name, order)
    s = ps.shade_batch(orc, m["b"], samples_seeded, m["sets"]["exposed"])
    assert np.array_equal(s["hit"]["prim"], m["sets"]["exposed"][2]["prim"])
    shade_every_way(m["scene"], s, ps.NB_LIGHT, "%s %s exposed" % (name, order))
    got, hits = m["scene"].shade_rays(s["origins"], s["directions"], keep_order=True, want_hits=True)
    qs.check_hits(hits, m["sets"]["exposed"][2], None, "%s %s shade_rays' hit records" % (name, order))


# ---------------------------------------------------------------------------------------------- 1 x 1 frames
@pytest.mark.parametrize("name,order", CASES)
def test_one_pixel_frames(rtx, orc, samples_half, name, order):
    """one pixel is one lane: rtx_render_rows (with and without statistics), rtx_render_view with hit records,
    rtx_render_view_rows, all against the oracle scene of that camera.  rtx_render_view walks the library's own stream,
    which the light orders: it also renders the frame under the ray sets' light, where that stream has the wall first."""
    f = ps.frame(rtx, orc, samples_half, name, order)
    b = f["b"]
    what = "%s %s" % (name, order)
    seen = rtx.Scene.view(1, 1, rect=(0, 0, 1, 1), **{k: b.kw[k] for k in ("eye", "look_at", "up", "distance")})
    with rtx.Scene(*f["seen"].args, **f["seen"].kw) as scene:
        for stats in (True, False):
            res = scene.render_view(seen, stats=stats, want_hits=True)
            qs.check_hits(res[1].reshape(-1), f["exp"], None, what + ": rtx_render_view under the ray sets' light")
            assert np.array_equal(res[0], f["seen_ref"]), what + ": rtx_render_view under the ray sets' light"
        assert np.array_equal(gpu_forms.render_both(scene)[0], f["seen_ref"]), what + ": rtx_render_rows under the ray sets' light"
    with rtx.Scene(*b.args, **b.kw) as scene:
        img, st = gpu_forms.render_both(scene)
        assert img.shape == (1, 1, 3)
        assert np.array_equal(img, f["ref"]), "%s: rtx_render_rows gives %s, the oracle %s (without the triangle: %s)" \
            % (what, img[0, 0].tolist(), f["ref"][0, 0].tolist(), f["without"][0, 0].tolist())
        assert st["primary_rays"] == 1 and st["primary_hits"] == 1 and st["shadow_rays"] == f["stats"]["shadow_rays"], (what, st)
        view = rtx.Scene.view(1, 1, rect=(0, 0, 1, 1), **{k: b.kw[k] for k in ("eye", "look_at", "up", "distance")})
        for stats in (True, False):
            res = scene.render_view(view, stats=stats, want_shade=True, want_hits=True)
            rgb, shade, hits = res[0], res[1], res[2]
            qs.check_hits(hits.reshape(-1), f["exp"], None, what + ": rtx_render_view's hit record")
            assert np.array_equal(rgb, f["ref"]) and np.array_equal(shade["rgb8"], rgb), what + ": rtx_render_view"
            rows = scene.render_view_rows(view, stats=stats)
            rows = rows[0] if stats else rows
            assert np.array_equal(rows, f["ref"]), what + ": rtx_render_view_rows gives %s" % rows[0, 0].tolist()
        assert np.array_equal(scene.render_view(view), f["ref"])
