"""The order in which the shading pass walks a batch's light samples (csrc/scene_prep.cpp: light_tour_order; read back
through rtx_scene_light_order).  Host only: no device is touched.

The order is free as far as the image goes — a sample's result lands in the sample's own column and a pixel's additions
run by ascending sample index — but it has to be a permutation of every batch that starts with the batch's first sample
(probe_kernel's kept answers are "walk position 0 of batch 0"), the same for the same inputs, and short."""
import importlib
import os

import numpy as np
import pytest

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIGHT_BATCH = 128                                  # scene_prep.h: RTX_LIGHT_BATCH
ONE_TRI = np.array([[-1.0, 1.0, -1.0, 1.0, 1.0, -1.0, 0.0, 1.0, 1.0]], F)
ONE_RGB = np.array([[0.5, 0.5, 0.5]], F)


@pytest.fixture(scope="module")
def rtx():
    return importlib.import_module("ray-tracer-rust_amd")


@pytest.fixture(scope="module")
def samples(rtx):
    return rtx.gen_samples()


def batches(nb_light):
    step = min(nb_light, LIGHT_BATCH)
    return [(b0, min(step, nb_light - b0)) for b0 in range(0, nb_light, step)]


def assert_batchwise_permutation(order, nb_ray, nb_light):
    order = order.reshape(nb_ray, nb_light)
    for r in range(nb_ray):
        for b0, bc in batches(nb_light):
            part = order[r, b0:b0 + bc]
            assert part[0] == b0, "ray %d batch at %d: position 0 must be the batch's first sample, is %d" % (r, b0, part[0])
            assert sorted(part.tolist()) == list(range(b0, b0 + bc)), "ray %d batch at %d is not a permutation of its indices" % (r, b0)


def order_of(rtx, samples, nb_ray, nb_light, light_tri=None):
    kw = {} if light_tri is None else dict(light_tri=light_tri)
    with rtx.Scene(16, 16, ONE_TRI, ONE_RGB, samples, nb_ray=nb_ray, nb_light_sample=nb_light, **kw) as s:
        assert s.info()["n_light_points"] == nb_ray * nb_light
        return s.light_order(), s.light_points()


@pytest.mark.parametrize("nb_ray", [1, 2])
@pytest.mark.parametrize("nb_light", [1, 2, 3, 100, 128, 129, 130, 257])
def test_every_batch_is_a_permutation_that_starts_with_its_first_sample(rtx, samples, nb_light, nb_ray):
    """129 and 257 leave a batch of ONE sample behind a full one, 130 a batch of two; and two scenes created from the
    same inputs walk in the same order."""
    order, _ = order_of(rtx, samples, nb_ray, nb_light)
    assert order.dtype == np.uint32 and order.shape == (nb_ray * nb_light,)
    assert_batchwise_permutation(order, nb_ray, nb_light)
    again, _ = order_of(rtx, samples, nb_ray, nb_light)
    assert (order == again).all(), "the order differs between two scenes of the same inputs"


@pytest.mark.parametrize("light", ["degenerate", "nan vertex", "infinite vertex"])
def test_a_light_without_usable_distances_still_gives_a_permutation(rtx, samples, light):
    """All three vertices equal: the points differ by the sampler's roundings at most, most distances are exactly 0 and
    tie.  A NaN or an infinite vertex: distances that are NaN or infinite win no comparison."""
    tri = {"degenerate": np.array([3.0, 9.0, -2.0] * 3, F),
           "nan vertex": np.array([-10.0, 300.0, -10.0, np.nan, 300.0, -10.0, 0.0, 300.0, 0.0], F),
           "infinite vertex": np.array([-10.0, 300.0, -10.0, 10.0, np.inf, -10.0, 0.0, 300.0, 0.0], F)}[light]
    for nb_light in (100, 130):
        order, _ = order_of(rtx, samples, 1, nb_light, light_tri=tri)
        assert_batchwise_permutation(order, 1, nb_light)


def path_length(points):
    return float(np.sqrt((np.diff(points.astype(np.float64), axis=0) ** 2).sum(axis=1)).sum())


def test_the_default_scenes_tour_is_a_quarter_of_the_index_order_path_at_most(rtx, samples):
    """main()'s light and sample table, 100 samples: the tour (nearest neighbour from sample 0, then 2-opt) must be at
    most a quarter as long as the path through the samples in index order — a floor on quality; random points of a
    triangle give 0.13 - 0.17 in simulation.  Measured for the default scene: 0.100 (index order 2531.0, tour 253.4)."""
    with rtx.default_scene([os.path.join(ROOT, "models", "bunny.obj")], 16, 16, samples) as s:
        pts, order = s.light_points(), s.light_order()
    assert len(pts) == 100
    assert_batchwise_permutation(order, 1, 100)
    index_path, tour = path_length(pts), path_length(pts[order])
    print("index-order path %.4f, tour %.4f, ratio %.4f" % (index_path, tour, tour / index_path))
    assert tour <= 0.25 * index_path
