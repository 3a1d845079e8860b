"""GPU parity of rtx_shade_rays (and its device-resident variant) against shade_sets.oracle_shade — render_pixel composed
from the CPU oracle's pieces, pinned to the oracle's own render_pixel by tests/test_shade_sets.py: the bits of the linear
colour, the RGB8 bytes, the hit count, and the hit records rtx_trace_rays writes for the same rays.  Every set is shaded
in the caller's order, in the default mode and with the regrouping pass forced, with and without statistics: all six
calls must give the same bytes.  The tolerance is zero."""
import importlib
import os

import numpy as np
import pytest

import query_sets as qs
import shade_sets as ss
from query_sets import H, NO_HIT, W, bits

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def rtx():
    mod = importlib.import_module("ray-tracer-rust_amd")
    assert mod.device_count() >= 1, "no HIP device: the product path has no CPU fallback"
    return mod


@pytest.fixture(scope="module")
def bunny(rtx, orc, samples_seeded):
    sets = ss.bunny_sets(orc, samples_seeded)
    scene = rtx.default_scene([os.path.join(ROOT, "models", "big_bunny.obj")], W, H, samples_seeded)
    assert scene.info()["n_tris"] == 4969 and scene.info()["n_ref_nodes"] != 0
    yield dict(scene=scene, sets=sets, nb_light=rtx.NB_LIGHT_SAMPLE)
    scene.close()


@pytest.fixture(scope="module")
def soup(rtx, orc, samples_seeded):
    sets = ss.soup_sets(orc, samples_seeded)
    a = sets["a"]
    scenes = {nb: rtx.Scene(*a["args"], nb_ray=nb, **a["kw"]) for nb in (1, 2)}
    yield dict(scenes=scenes, sets=sets, nb_light=a["kw"]["nb_light_sample"])
    for s in scenes.values():
        s.close()


def shade_every_way(scene, s, nb_light, what):
    """caller's order, default, forced regrouping x with / without statistics: the oracle's answer, the same bytes; the hit
    records are rtx_trace_rays'; returns the statistics of the caller's-order call"""
    o, d, exp = s["origins"], s["directions"], s["shade"]
    traced = scene.trace_rays(o, d, keep_order=True)
    assert np.array_equal(traced["prim"], s["hit"]["prim"]), what
    n_hits = int((s["hit"]["prim"] != NO_HIT).sum())
    first = kept = None
    for mode in (dict(keep_order=True), dict(), dict(force_regroup=True)):
        for stats in (False, True):
            res = scene.shade_rays(o, d, want_hits=True, stats=stats, **mode)
            got, hits = res[0], res[1]
            tag = "%s %s stats=%s" % (what, mode, stats)
            if stats:
                st = res[2]
                assert st["primary_rays"] == len(o) and st["primary_hits"] == n_hits, (tag, st)
                assert st["shadow_rays"] == nb_light * n_hits and st["rays"] == st["primary_rays"] + st["shadow_rays"], (tag, st)
                kept = st if kept is None else kept
            assert len(got) == len(exp), tag
            bad = np.nonzero((bits(got["linear"]) != bits(exp["linear"])).any(axis=1))[0]
            assert not len(bad), "%s: linear differs at pixels %s: %s != %s" % (tag, bad[:8], got["linear"][bad[:3]], exp["linear"][bad[:3]])
            assert np.array_equal(got["rgb8"], exp["rgb8"]), tag + ": rgb8 differs"
            assert np.array_equal(got["hits"], exp["hits"]), tag + ": hits differ"
            assert hits.tobytes() == traced.tobytes(), tag + ": the hit records are not rtx_trace_rays'"
            first = got if first is None else first
            assert got.tobytes() == first.tobytes(), tag + " differs from the first call"
    assert scene.shade_rays(o, d).tobytes() == first.tobytes(), what + ": without out_hits"
    return kept


@pytest.mark.parametrize("name", ["camera", "random", "penumbra", "far"])
def test_bunny_sets(bunny, name):
    shade_every_way(bunny["scene"], bunny["sets"][name], bunny["nb_light"], name)


def test_both_pipelines_give_the_camera_set_the_same_bytes(bunny):
    """pixel k of the set is (px, py) = (k % W, k // W): put_pixel's byte order (main.rs:293-294); the sample index inside
    create_rays is px * width + py"""
    s = bunny["sets"]["camera"]
    got = bunny["scene"].shade_rays(s["origins"], s["directions"])
    assert np.array_equal(got["rgb8"].reshape(H, W, 3), bunny["scene"].render_rows())


def test_a_hard_ray_beside_regular_ones(bunny):
    s = bunny["sets"]["hard"]
    st = shade_every_way(bunny["scene"], s, bunny["nb_light"], "hard")
    assert st["redo_tiles"] >= 1
    twin = bunny["sets"]["hard_twin"]
    got = bunny["scene"].shade_rays(twin["origins"], twin["directions"])
    assert got.tobytes() == twin["shade"].tobytes() and got["hits"][0] == 1


@pytest.mark.parametrize("n", [1, 63, 64, 65])
def test_batch_sizes_around_one_wavefront(bunny, n):
    s = ss.take(bunny["sets"]["random"], np.arange(n))
    shade_every_way(bunny["scene"], s, bunny["nb_light"], "random[:%d]" % n)


@pytest.mark.parametrize("nb_ray", [1, 2])
def test_soup_with_spheres(soup, nb_ray):
    s = soup["sets"][nb_ray]
    shade_every_way(soup["scenes"][nb_ray], s, soup["nb_light"], "soup nb_ray=%d" % nb_ray)
    got, hits = soup["scenes"][nb_ray].shade_rays(s["origins"], s["directions"], want_hits=True)
    a = soup["sets"]["a"]
    qs.check_normals(hits, s["hit"], soup["scenes"][nb_ray].normals(), a["kinds"], "soup nb_ray=%d" % nb_ray)


@pytest.mark.parametrize("n", [1, 32, 33])
def test_batch_sizes_with_two_rays_per_pixel(soup, n):
    s = ss.take(soup["sets"][2], np.arange(n))
    assert len(s["origins"]) == 2 * n
    shade_every_way(soup["scenes"][2], s, soup["nb_light"], "soup nb_ray=2 [:%d]" % n)


def test_an_entry_is_keyed_by_its_ray_0(soup, orc, samples_seeded):
    """128 pixels of two rays on the soup: ray 0 of every odd pixel is hard (-0.0 in y) and leaves the plane z = 0, in
    front of the soup, along +z — away from it, a miss; every other ray is a regular ray of set A.  The key's bit 31
    gathers hard entries and an entry's key comes from its ray 0 (rtxq::key_kernel, stride nb_ray), so the 64 odd pixels
    share one wavefront after the regrouping pass: one reference walk, against two in the caller's order, where each of
    the two wavefronts holds 32 of them.  A key read from flat ray i instead of ray i * nb_ray would call the pixels
    2, 6, 10 ... hard — all regular — and leave the odd pixels in both wavefronts: two reference walks."""
    a = soup["sets"]["a"]
    so, sd, _, _ = qs.set_a(orc, samples_seeded)["trace"]
    o, d = so[:256].copy(), sd[:256].copy()
    odd_ray0 = np.arange(2, 256, 4)
    o[odd_ray0, 2] = 0.0
    d[odd_ray0] = (0.0, -0.0, 1.0)
    assert a["hi"][2] < 0.0 and np.abs(o[odd_ray0]).max() <= a["bound"]         # outside the soup, inside the origin bound
    s = ss.shade_set(orc, soup["sets"]["osc2"], o, d, 2, soup["nb_light"], a["kw"]["light_tri"], samples_seeded,
                     soup["sets"]["tables"])
    assert len(s["shade"]) == 128 and (s["hit"]["prim"][odd_ray0] == NO_HIT).all()
    assert (s["hit"]["prim"][1::2] != NO_HIT).sum() >= 64                        # the other rays do meet the soup
    scene = soup["scenes"][2]
    walks = {}
    for name, mode in (("keep_order", dict(keep_order=True)), ("force_regroup", dict(force_regroup=True))):
        got, st = scene.shade_rays(o, d, stats=True, **mode)
        print(name, "redo_tiles", st["redo_tiles"])
        walks[name] = st["redo_tiles"]
        assert got.tobytes() == s["shade"].tobytes(), name
    assert walks == dict(keep_order=2, force_regroup=1), walks


def test_a_batch_above_the_regrouping_threshold_with_default_flags(bunny):
    """the random set repeated and shuffled to 18,000 pixels (> 16,384): with flags = 0 the batch takes the regrouping pass"""
    base = bunny["sets"]["random"]
    order = np.random.default_rng(3).permutation(np.tile(np.arange(256), 71))[:18000]
    s = ss.take(base, order)
    scene = bunny["scene"]
    got, st = scene.shade_rays(s["origins"], s["directions"], stats=True)
    kept = scene.shade_rays(s["origins"], s["directions"], keep_order=True)
    assert got.tobytes() == kept.tobytes()
    assert got.tobytes() == s["shade"].tobytes()
    n_hits = int((s["hit"]["prim"] != NO_HIT).sum())
    assert st["primary_rays"] == 18000 and st["primary_hits"] == n_hits and st["shadow_rays"] == 100 * n_hits


def test_device_resident_call_on_a_stream_of_its_own(rtx, bunny):
    torch = pytest.importorskip("torch")
    assert torch.cuda.is_available(), "torch sees no GPU"
    scene = bunny["scene"]
    s = bunny["sets"]["random"]
    o, d = s["origins"], s["directions"]
    n = len(o)
    stream = torch.cuda.Stream(device="cuda:0")
    assert stream.cuda_stream != torch.cuda.default_stream().cuda_stream
    with torch.cuda.stream(stream):
        t_o = torch.from_numpy(o).to("cuda:0")
        t_d = torch.from_numpy(d).to("cuda:0")
        shade = torch.full((n * 16 + 16,), 0xAA, dtype=torch.uint8, device="cuda:0")
        hits = torch.full((n * 32,), 0xAA, dtype=torch.uint8, device="cuda:0")
        assert shade.data_ptr() % 16 == 0
        with pytest.raises(rtx.RtxError) as e:
            scene.shade_rays_device(0, n, t_o.data_ptr(), t_d.data_ptr(), shade.data_ptr() + 8, None, stream.cuda_stream)
        assert e.value.code == rtx.ERR_BAD_ARG
        for mode in (dict(keep_order=True), dict(force_regroup=True)):
            scene.shade_rays_device(0, n, t_o.data_ptr(), t_d.data_ptr(), shade.data_ptr(), hits.data_ptr(),
                                    stream.cuda_stream, **mode)
            # a host call right behind it uses the same sort buffers on the library's stream
            host, host_hits = scene.shade_rays(o, d, want_hits=True, force_regroup=True)
            stream.synchronize()
            out = shade.cpu().numpy()
            assert out[:n * 16].tobytes() == host.tobytes() == s["shade"].tobytes(), mode
            assert (out[n * 16:] == 0xAA).all()
            assert hits.cpu().numpy().tobytes() == host_hits.tobytes(), mode
            shade.fill_(0xAA)
            hits.fill_(0xAA)
        scene.shade_rays_device(0, n, t_o.data_ptr(), t_d.data_ptr(), shade.data_ptr(), None, stream.cuda_stream)
        stream.synchronize()
        assert shade.cpu().numpy()[:n * 16].tobytes() == s["shade"].tobytes()
    # shading leaves the render workspace alone
    cam = bunny["sets"]["camera"]
    assert np.array_equal(scene.render_rows(), cam["shade"]["rgb8"].reshape(H, W, 3))
