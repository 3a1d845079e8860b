"""The shadow walk's distance certificate (csrc/rtx_traverse.hpp: candidate_occludes_voted) against the expression it
stands for (candidate_occludes: main.rs:220-221 on bvh.rs:69's hit point), both restated in numpy float32
(tests/occluder_sets.py).  No GPU.

    fma(t, 1 + 2^-20,  cs) <= limit   must imply   !(f(t) > limit)        cs = 2^-22 (|ox| + |oy| + |oz|)
    fma(t, 1 - 2^-20, -cs) >  limit   must imply     f(t) > limit         f(t) = |o - fl(o + fl(t d))|

on 12 million rays: origins from 0 to 3e4 in magnitude, t from 1 to 3e4 (and within two ulp of 1.0, the leaf rule's
bound), one direction component scaled by 1e-6, and limits placed around f(t) itself — within 40 ulp, and within 2^-17
relative, where the margins of the certificate end."""
import numpy as np
import pytest

import np_ref
import occluder_sets as oc
import shade_sets as ss

F = np.float32
CHUNK = 1 << 20


def rays(rng, n, t_near_one=False):
    """origins, unit directions (Ray::new's arithmetic) and distances of one chunk"""
    mag = np.exp(rng.uniform(np.log(1e-2), np.log(3e4), size=(n, 1)))
    o = (rng.uniform(-1.0, 1.0, size=(n, 3)) * mag).astype(F)
    o[rng.random(n) < 0.02] = 0.0                                      # the world's origin itself
    o[np.arange(n), rng.integers(0, 3, n)] *= (rng.random(n) < 0.8)     # and a zero coordinate
    v = rng.normal(size=(n, 3))
    v[np.arange(n), rng.integers(0, 3, n)] *= 1e-6
    v = v.astype(F)
    d = np.stack(np_ref._normalize(np_ref._v(v)), axis=-1)
    if t_near_one:
        t = (F(1.0) + rng.integers(0, 3, n).astype(F) * np.spacing(F(1.0))).astype(F)
    else:
        t = np.exp(rng.uniform(0.0, np.log(3e4), size=n)).astype(F)
    return o, d, t


def f_of_t(o, d, t):
    q = [o[:, c] - (o[:, c] + t * d[:, c]) for c in range(3)]
    return np.sqrt(np_ref._dot(q, q))


def step_ulps(x, k):
    """x moved by k float32 steps (positive finite x)"""
    return (x.view(np.int32) + k.astype(np.int32)).view(F)


FAMILIES = {
    # name: (chunks, t near one, how the limit is placed around f(t))
    "within 40 ulp": (4, False, lambda rng, f: step_ulps(f, rng.integers(-40, 41, len(f)))),
    "within 2^-17": (4, False, lambda rng, f: (f * (F(1.0) + rng.uniform(-2.0 ** -17, 2.0 ** -17, len(f)).astype(F))).astype(F)),
    "t within 2 ulp of 1": (2, True, lambda rng, f: step_ulps(f, rng.integers(-40, 41, len(f)))),
    "t within 2 ulp of 1, 2^-17": (2, True, lambda rng, f: (f * (F(1.0) + rng.uniform(-2.0 ** -17, 2.0 ** -17, len(f)).astype(F))).astype(F)),
}


@pytest.fixture(scope="module")
def tallies():
    """per family: rays, wrong verdicts, and the counts of yes / no / undecided — every family is run once"""
    out = {}
    for k, (name, (chunks, near_one, place)) in enumerate(FAMILIES.items()):
        rng = np.random.default_rng(900 + k)
        n = wrong = yes_n = no_n = 0
        for _ in range(chunks):
            o, d, t = rays(rng, CHUNK, near_one)
            f = f_of_t(o, d, t)
            ok = f > 0
            limit = np.where(ok, place(rng, np.where(ok, f, F(1.0))), f)
            exact = oc.exact_occludes(o, d, t, limit)
            yes, no = oc.certificate(o, t, limit)
            wrong += int((yes & ~exact).sum()) + int((no & exact).sum()) + int((yes & no).sum())
            n, yes_n, no_n = n + len(t), yes_n + int(yes.sum()), no_n + int(no.sum())
        out[name] = dict(n=n, wrong=wrong, yes=yes_n, no=no_n, undecided=n - yes_n - no_n)
        print("%-28s %9d rays: yes %5.1f %%  no %5.1f %%  undecided %5.1f %%  wrong %d"
              % (name, n, 100.0 * yes_n / n, 100.0 * no_n / n, 100.0 * (n - yes_n - no_n) / n, wrong))
    return out


def test_the_certificate_never_contradicts_the_exact_answer(tallies):
    assert sum(v["n"] for v in tallies.values()) >= 10_000_000
    for name, v in tallies.items():
        assert v["wrong"] == 0, (name, v)


def test_the_near_boundary_family_sees_every_verdict(tallies):
    """a condition on the inputs: limits within 2^-17 of f(t) lie on both sides of both margins"""
    v = tallies["within 2^-17"]
    for k in ("yes", "no", "undecided"):
        assert v[k] * 10 >= v["n"], (k, v)


def test_special_values_land_in_the_exact_test():
    """a NaN in t, the origin or the limit, an infinite origin and t = limit fail both comparisons; an infinite t or
    limit is settled as the expression settles it for a direction without a zero component (the walks that use the
    certificate hold no other)"""
    nan, inf = F(np.nan), F(np.inf)
    o = np.array([[1.0, 2.0, 3.0], [nan, 2.0, 3.0], [inf, 2.0, 3.0], [1.0, -inf, 3.0], [1.0, 2.0, 3.0], [1.0, 2.0, 3.0]], F)
    t = np.array([nan, 5.0, 5.0, 5.0, 5.0, 5.0], F)
    limit = np.array([9.0, 9.0, 9.0, 9.0, nan, 5.0], F)
    yes, no = oc.certificate(o, t, limit)
    assert not yes.any() and not no.any()
    d = np.array([[0.6, -0.48, 0.64]] * 4, F)
    o = np.array([[1.0, 2.0, 3.0]] * 4, F)
    t = np.array([inf, inf, 5.0, 1.0], F)
    limit = np.array([9.0, inf, inf, inf], F)
    yes, no = oc.certificate(o, t, limit)
    exact = oc.exact_occludes(o, d, t, limit)
    assert list(exact) == [False, True, True, True]
    assert list(yes) == [False, True, True, True] and list(no) == [True, False, False, False]


def test_the_restated_expression_is_the_oracles_own_distance_test(orc, samples_seeded):
    """The oracle's render_pixel with ONE light sample: a hit pixel is black iff the oracle's own distance test
    (main.rs:220) calls its one shadow ray occluded.  On 64 x 64 pixels of the `coplanar` fixture — candidates within
    ulps of the light's distance, both answers — the numpy restatement on the oracle's closest hit says the same."""
    f = oc.fixture("coplanar")
    W = H = 64
    kw = dict(f["kw"], distance=48.0, nb_light_sample=1)
    osc = orc.Scene(W, H, f["tris"], f["rgb"], samples_seeded, **kw)
    image, _ = osc.render_rows(mode=orc.MODE_BVH)
    o, raw, _, _, _ = ss.camera_raw_rays(orc, W, H, kw["eye"], kw["look_at"], kw["up"], kw["distance"], samples_seeded)
    prim, _, orig = ss._closest(osc, o, ss.units_of(orc, raw))
    assert (prim == 1).all(), "every pixel sees the wall"
    lp = ss.light_points(orc, oc.LIGHT, samples_seeded, 1, 1)[0, 0]
    to_light = (lp[None, :] - orig).astype(F)
    unit = ss.units_of(orc, to_light)
    sprim, t, _ = ss._closest(osc, orig, unit)
    osc.close()
    assert (sprim == 0).all(), "every shadow ray meets the triangle in the light's plane"
    occluded = oc.exact_occludes(orig, unit, t, np_ref._norm(np_ref._v(to_light)))
    black = (image.reshape(-1, 3).max(axis=1) == 0)
    assert black.sum() >= 400 and (~black).sum() >= 400
    assert np.array_equal(occluded, black)
