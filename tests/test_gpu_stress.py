"""Randomised parity: scenes with random cameras, lights, primitive mixes, frame sizes, ray counts — everything the
shorter-than-IEEE sequences, the cost-ordered schedule and the up-front leaves see differently from the fixed goldens.
Each scene is rendered by the oracle (faithful BVH) and through the C ABI; bytes and hit counts must be equal.
RTX_STRESS_SCENES scales it up for a soak (default 16 scenes, a few seconds)."""
import importlib
import os

import numpy as np
import pytest

from gpu_forms import render_both
from sequence_model import random_scene

pytestmark = pytest.mark.gpu
F = np.float32


@pytest.fixture(scope="module")
def rtx():
    mod = importlib.import_module("ray-tracer-rust_amd")
    assert mod.device_count() >= 1, "no HIP device: the product path has no CPU fallback"
    return mod


def test_random_scenes_match_the_oracle(rtx, orc, samples_seeded):
    n_scenes = int(os.environ.get("RTX_STRESS_SCENES", "16"))
    rng = np.random.default_rng(20261004)
    checked = hits = 0
    for k in range(n_scenes):
        W, H, tris, rgb, spheres, srgb, kinds, kw = random_scene(rng)
        extra = dict(spheres=spheres, sphere_rgb=srgb, kinds=kinds) if len(spheres) else {}
        ref, ost = orc.Scene(W, H, tris, rgb, samples_seeded, **extra, **kw).render_rows(mode=orc.MODE_BVH)
        if ost["nonfinite_t"]:
            continue                                            # outside the parity contract
        with rtx.Scene(W, H, tris, rgb, samples_seeded, **extra, **kw) as s:
            img, st = render_both(s)
        assert st["primary_hits"] == ost["primary_hits"], "scene %d: %r" % (k, kw)
        assert np.array_equal(img, ref), "scene %d: %d bytes differ (%dx%d, %d tris, %d spheres, %r)" % (
            k, int((img != ref).sum()), W, H, len(tris), len(spheres), kw)
        checked += 1
        hits += ost["primary_hits"]
    assert checked >= n_scenes * 3 // 4 and hits > 100 * checked
