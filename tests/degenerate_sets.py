"""Scenes, poses and rays in which zero-area triangles take part, with the CPU oracle's answers: numpy, the oracle binding
and the library's host side only, no GPU.

A zero-area triangle is one of six forms, in two classes:
    Z  exactly singular: "point" (v0 = v1 = v2), "e1zero" (v1 = v0), "e2zero" (v2 = v0).  Moeller-Trumbore's determinant is
       exactly +-0 for every ray and the |det| < 1e-5 gate always rejects (triangle.rs:73): never hit.
    C  collinear, the determinant rounding noise of order |e|^2 |d| 2^-24, which for edges of tens of units passes the gate:
       "C1" (v1 = v2, so e1 = e2), "C2" (a, a + e, a + 2e, on a grid on which the sums are exact) and "C3"
       (a, fl((a + b) / 2), b).  C1 and C2 have cross(e1, e2) exactly zero in float32 and Triangle::new's normal is 0/0;
       C3 has a finite unit normal that means nothing.  Rays aimed at such a segment are accepted now and then, with a
       finite t that means nothing either.

The scenes: "thicket" — big_bunny (every 19th triangle left out, so that the scene stays below big_bunny + ground's
size) + ground, 40 triangles of each form at fixed Vec positions between the mesh's, a C2 needle across the whole ground
plane, a zero-radius sphere and an ordinary one, 64 x 48 through view_sets' "side" camera with 8 light samples; "soup" —
query_sets.scene_a's soup with 30 % of its triangles replaced by the six forms; and the size scenes (an ordinary
triangle and n point triangles at one point, segments on one line, points).  Poses of the thicket: collapse, fold, unfold,
prims_all.  Ray sets: "exposed" (the oracle names a C triangle, t > 1, MODE_BVH and MODE_BRUTE alike), "grazing" (aimed the
same way, answered with something else or a miss), "mixed".  Every ray is a point pair (origin, target): its direction is
fl(target - origin), so the occlusion pair of a ray walks exactly the ray's direction.

tests/test_degenerate_sets.py states, without a GPU, the conditions these fixtures must meet; tests/test_degenerate_host.py
and tests/test_gpu_degenerate.py use them.  Everything is drawn from fixed seeds and built once per process
(query_sets._once)."""
import numpy as np

import prune_sets as ps
import query_sets as qs
import shade_sets as ss
import view_sets as vs
from query_sets import F, NO_HIT

FORMS = ("point", "e1zero", "e2zero", "C1", "C2", "C3")
Z_FORMS, C_FORMS, NAN_FORMS = (0, 1, 2), (3, 4, 5), (0, 1, 2, 3, 4)      # NAN_FORMS: Triangle::new's normal is 0/0
N_PER_FORM = 40
LEFT_OUT = 19                                         # every 19th triangle of the mesh is left out
NEEDLE = np.array([-9000.0, 0.5, -9000.0, 0.0, 0.5, 0.0, 9000.0, 0.5, 9000.0], F)       # C2: (a, a + e, a + 2e), exact
NEEDLE_NUMBER = 7                                     # its triangle number
SPHERE_AT = (1000, 3000)                              # Vec positions of the spheres
SPHERES = np.array([[-40.0, 150.0, 30.0, 0.0], [105.0, 32.0, 20.0, 32.0]], F)            # a zero radius, an ordinary one
SPHERE_RGB = np.array([[0.9, 0.2, 0.2], [0.3, 0.5, 0.9]], F)
FORM_RGB = np.array([[0.9, 0.1, 0.1], [0.1, 0.9, 0.1], [0.1, 0.1, 0.9], [0.9, 0.8, 0.1], [0.1, 0.8, 0.9], [0.9, 0.2, 0.8]], F)
SIDE = vs.BUNNY_VIEWS["side"]
THICKET_VIEW = ((64, 48), SIDE[1], SIDE[2], 44.0)        # the side view's field: its distance 30 at 44 columns
NB_LIGHT = 8
EDGE_MIN, EDGE_MAX = 10.0, 60.0
SOUP_SHARE = 0.3
SOUP_EDGE_MIN, SOUP_EDGE_MAX = 15.0, 40.0             # the soup's box is 16 units wide: its C segments reach through it
N_SET = 128
MIN_PER_CLASS = 8
BUDGET = 60000                                        # aimed rays tried per search, at the most
REACH = 8.0                                           # a ray's target: origin + REACH (aimed point - origin)
N_ORDINARY = 384
SIZES = (1, 31, 32, 33, 255, 256, 257)
ONE_POINT = (3.0, 4.0, -12.0)
FRAME_BUDGET, N_FRAMES = 20000, 4
POSES = ("collapse", "fold", "unfold", "prims_all")
N_FOLDED = 200
HEAD_ABOVE = 150.0                                    # the head: triangles of the mesh with every vertex above this height
FAR_AWAY = (0.0, -5000.0, 0.0, 1.0, -5000.0, 0.0, 0.0, -5000.0, 1.0)
# a C2 and a point triangle as lights.  Triangle::get_sample's weights do not sum to one (triangle.rs:113-127), so the first's
# samples lie in the plane through the origin and the segment and the second's are multiples of the point
LIGHTS = {"segment": (-30.0, 300.0, -10.0, 0.0, 300.0, 0.0, 30.0, 300.0, 10.0), "point": (5.0, 280.0, -15.0) * 3}


# ---------------------------------------------------------------------------------------------------------- the forms
def triangle_new(orc, t):
    """(e1, e2, normal) of Triangle::new by the oracle"""
    e1, e2, n = np.zeros(3, F), np.zeros(3, F), np.zeros(3, F)
    t = np.ascontiguousarray(t, F).reshape(9)
    orc.lib().orc_triangle_new(orc._fp(t[0:3].copy()), orc._fp(t[3:6].copy()), orc._fp(t[6:9].copy()), orc._fp(e1), orc._fp(e2), orc._fp(n))
    return e1, e2, n


def cross32(a, b):
    """cross(a, b) in float32, each product and difference rounded (vec3.rs)"""
    a, b = np.asarray(a, F), np.asarray(b, F)
    return np.array([a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]], F)


def draw(orc, rng, form, lo, hi, edge_min, edge_max):
    """one triangle of the form inside the box [lo, hi] -> float32 [9]"""
    while True:
        a, b = rng.uniform(lo, hi).astype(F), rng.uniform(lo, hi).astype(F)
        if form in Z_FORMS:
            return np.concatenate([(a, a, a), (a, a, b), (a, b, a)][form]).astype(F)
        length = float(np.linalg.norm(b.astype(np.float64) - a))
        if not edge_min <= length <= edge_max:
            continue
        if form == 3:
            return np.concatenate([a, b, b]).astype(F)
        if form == 4:                                 # on a grid of 2^-8: a + e and a + 2e are exact, e2 = 2 e1 exactly
            a = (np.round(a.astype(np.float64) * 256.0) / 256.0).astype(F)
            e = (np.round((b.astype(np.float64) - a) * 128.0) / 256.0).astype(F)
            return np.concatenate([a, a + e, a + F(2.0) * e]).astype(F)
        t = np.concatenate([a, ((a + b) * F(0.5)).astype(F), b]).astype(F)
        if np.isfinite(triangle_new(orc, t)[2]).all():
            return t


def segment_of(t):
    """the two end points of a C triangle's segment"""
    v = np.asarray(t, F).reshape(3, 3)
    return v[0], v[2]


# ---------------------------------------------------------------------------------------------------------- the thicket
def thicket(orc):
    """dict(tris [n, 9], rgb, spheres, sphere_rgb, kinds, form = per triangle number -1 (ordinary) or the form's index, at =
    Vec position per triangle number, form_at = the same per Vec position (-1 for a sphere), ground, needle = triangle
    numbers, mesh_lo / mesh_hi)"""
    def make():
        mesh = orc.import_obj(orc.model_path("big_bunny.obj"))
        mesh = mesh[np.arange(len(mesh)) % LEFT_OUT != LEFT_OUT - 1]
        lo, hi = mesh.reshape(-1, 3).min(axis=0), mesh.reshape(-1, 3).max(axis=0)
        n_deg = N_PER_FORM * len(FORMS)
        n = len(mesh) + n_deg + 2                                        # + the needle and the ground
        rng = np.random.default_rng(2026)
        places = np.setdiff1d(np.unique(np.linspace(12, n - 12, n_deg).astype(np.int64)), [NEEDLE_NUMBER])
        assert len(places) == n_deg
        form = np.full(n, -1, np.int8)
        form[places] = np.arange(n_deg) % len(FORMS)                     # interleaved: point, e1zero, ..., C3, point, ...
        tris = np.zeros((n, 9), F)
        for k in places:
            tris[k] = draw(orc, rng, int(form[k]), lo + 5.0, hi - 5.0, EDGE_MIN, EDGE_MAX)
        tris[NEEDLE_NUMBER], form[NEEDLE_NUMBER] = NEEDLE, 4
        tris[n - 1] = orc.GROUND_TRI
        ordinary = np.nonzero(form == -1)[0][:-1]
        tris[ordinary] = mesh
        rgb = np.ones((n, 3), F)
        rgb[form >= 0] = FORM_RGB[form[form >= 0]]
        rgb[n - 1] = orc.GROUND_RGB
        kinds = np.zeros(n + len(SPHERES), np.uint8)
        kinds[list(SPHERE_AT)] = 1
        at = np.nonzero(kinds == 0)[0]
        form_at = np.full(len(kinds), -1, np.int8)
        form_at[at] = form
        out = dict(tris=np.ascontiguousarray(tris), rgb=rgb, spheres=SPHERES.copy(), sphere_rgb=SPHERE_RGB.copy(), kinds=kinds,
                   form=form, at=at, form_at=form_at, ground=n - 1, needle=NEEDLE_NUMBER, mesh_lo=lo, mesh_hi=hi,
                   ordinary=ordinary)
        for a in out.values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        return out
    return qs._once("deg_thicket", make)


def scene_kw(prims, view=THICKET_VIEW, **more):
    """keywords both bindings' Scene take after (width, height, tris, rgb, samples)"""
    kw = dict(vs.camera(view), nb_light_sample=NB_LIGHT, spheres=prims["spheres"], sphere_rgb=prims["sphere_rgb"], kinds=prims["kinds"])
    kw.update(more)
    return kw


def oracle_scene(orc, samples, prims, view=THICKET_VIEW, **more):
    return orc.Scene(view[0][0], view[0][1], prims["tris"], prims["rgb"], samples, **scene_kw(prims, view, **more))


def open_scene(rtx, samples, prims, view=THICKET_VIEW, **more):
    """the library's scene of the same arguments"""
    return rtx.Scene(view[0][0], view[0][1], prims["tris"], prims["rgb"], samples, **scene_kw(prims, view, **more))


def render(orc, samples, prims, view=THICKET_VIEW, **more):
    """-> dict(osc, frame, stats, tri = the hit primitive per pixel (one ray's), lin)"""
    osc = oracle_scene(orc, samples, prims, view, **more)
    frame, st, tri, lin = osc.render_rows(mode=orc.MODE_BVH, want_tri=True, want_lin=True)
    for a in (frame, tri, lin):
        a.setflags(write=False)
    return dict(osc=osc, frame=frame, stats=st, tri=tri, lin=lin)


def tables_of(orc, prims):
    return ss.prim_tables(orc, prims["tris"], prims["rgb"], prims["spheres"], prims["sphere_rgb"], prims["kinds"])


def without(prims, forms):
    """the primitives with every triangle of the named forms taken far away (the primitive numbers stay)"""
    tris = prims["tris"].copy()
    tris[np.isin(prims["form"], forms)] = FAR_AWAY
    return dict(prims, tris=tris)


def thicket_frame(orc, samples):
    return qs._once("deg_thicket_frame", lambda: render(orc, samples, thicket(orc)))


def thicket_tables(orc):
    return qs._once("deg_thicket_tables", lambda: tables_of(orc, thicket(orc)))


# ---------------------------------------------------------------------------------------------------------- the soup
def soup(orc, samples):
    """query_sets.scene_a's soup with SOUP_SHARE of its triangles replaced by the six forms in turn: the same dict as
    thicket()'s, and `kw` = the view's keywords"""
    def make():
        a = qs.scene_a(orc, samples)
        _, _, tris, rgb, _ = a["args"]
        tris = tris.copy()
        rng = np.random.default_rng(2027)
        replaced = np.sort(rng.choice(len(tris), int(round(SOUP_SHARE * len(tris))), replace=False))
        form = np.full(len(tris), -1, np.int8)
        form[replaced] = np.arange(len(replaced)) % len(FORMS)
        lo, hi = np.array([-8.0, -8.0, -22.0]), np.array([8.0, 8.0, -6.0])
        for k in replaced:
            f = int(form[k])
            if f in C_FORMS:                          # a segment through the soup's centre region, longer than the soup is wide
                tris[k] = draw(orc, rng, f, lo - 12.0, hi + 12.0, SOUP_EDGE_MIN, SOUP_EDGE_MAX)
            else:
                tris[k] = draw(orc, rng, f, lo, hi, 0.0, 0.0)
        kinds = a["kinds"]
        at = np.nonzero(kinds == 0)[0]
        form_at = np.full(len(kinds), -1, np.int8)
        form_at[at] = form
        return dict(tris=np.ascontiguousarray(tris), rgb=rgb, spheres=a["kw"]["spheres"], sphere_rgb=a["kw"]["sphere_rgb"], kinds=kinds,
                    form=form, at=at, form_at=form_at, kw=dict(qs.SOUP_VIEW, spheres=a["kw"]["spheres"], sphere_rgb=a["kw"]["sphere_rgb"],
                                                                 kinds=kinds))
    return qs._once("deg_soup", make)


def soup_scene(binding, samples, prims, **more):
    """either binding's Scene of the soup, 32 x 32"""
    return binding.Scene(qs.W, qs.H, prims["tris"], prims["rgb"], samples, **dict(prims["kw"], **more))


def soup_frame(orc, samples, nb_ray=1):
    def make():
        osc = soup_scene(orc, samples, soup(orc, samples), nb_ray=nb_ray)
        frame, st, tri = osc.render_rows(mode=orc.MODE_BVH, want_tri=True)
        return dict(osc=osc, frame=frame, stats=st, tri=tri)
    return qs._once("deg_soup_frame_%d" % nb_ray, make)


# ---------------------------------------------------------------------------------------------------------- size scenes
def size_scenes():
    """name -> dict(tris, pose = every triangle onto ONE_POINT, back = the scene's own vertices)"""
    def make():
        out = {}
        one = np.array([[0, 0, -5, 4, 0, -5, 0, 4, -6]], F)
        p = np.asarray(ONE_POINT, F)
        for n in SIZES:
            out["one_and_%d_points" % n] = np.concatenate([one, np.tile(np.tile(p, 3), (n, 1))]).astype(F)
        k = np.arange(300, dtype=np.float64)[:, None]
        a, e = np.array([-40.0, 2.0, -30.0]), np.array([0.25, 0.125, -0.5])           # a + k e: exact in float32
        out["segments"] = np.concatenate([a + k * e, a + (k + 7.0) * e, a + (k + 3.0) * e], axis=1).astype(F)
        g = np.stack(np.meshgrid(np.arange(7.0), np.arange(7.0), np.arange(6.0), indexing="ij"), axis=-1).reshape(-1, 3)
        out["points"] = np.tile((g * 3.0 + np.array([-9.0, 1.0, -30.0])).astype(F), (1, 3))
        return {name: dict(tris=np.ascontiguousarray(t), pose=np.ascontiguousarray(np.tile(np.tile(p, 3), (len(t), 1)).astype(F)))
                for name, t in out.items()}
    return qs._once("deg_sizes", make)


def open_sized(rtx, samples, sc, **more):
    rgb = np.linspace(0.1, 1.0, 3 * len(sc["tris"]), dtype=F).reshape(-1, 3)
    return rtx.Scene(8, 8, sc["tris"], rgb, samples[:4096], nb_light_sample=4,
                     **dict(dict(reference_tree=rtx.REFTREE_NEVER, tie_rank=None, **axis_view()), **more))


def axis_view():
    return dict(eye=(0.0, 0.0, 0.0), look_at=(0.0, 0.0, -1.0), up=(0.0, 1.0, 0.0), distance=8.0,
                light_tri=(-2.0, 9.0, -3.0, 2.0, 9.0, -3.0, 0.0, 9.0, 1.0))


# ---------------------------------------------------------------------------------------------------------- the poses
def head(prims):
    """triangle numbers of the mesh's head: every vertex above HEAD_ABOVE"""
    y = prims["tris"][:, 1::3]
    return np.nonzero((prims["form"] == -1) & (y.min(axis=1) > HEAD_ABOVE) & (np.arange(len(y)) != prims["ground"]))[0]


def folded(prims):
    """triangle numbers `fold` makes C1: every 20th ordinary triangle of the mesh, the first N_FOLDED"""
    return prims["ordinary"][::20][:N_FOLDED]


def pose(orc, name):
    """the posed primitives, every array in full: the thicket's dict with tris (and for prims_all spheres, rgb, sphere_rgb)
    replaced, and `form` as the pose makes it"""
    def make():
        t = thicket(orc)
        p = dict(t, tris=t["tris"].copy(), form=t["form"].copy())
        if name in ("collapse", "prims_all"):
            h = head(t)
            point = t["tris"][h].reshape(-1, 3).astype(np.float64).mean(axis=0).astype(F)
            p["tris"][h] = np.tile(point, 3)
            p["form"][h] = 0
            if name == "prims_all":
                p["spheres"], p["rgb"], p["sphere_rgb"] = t["spheres"].copy(), t["rgb"].copy(), t["sphere_rgb"].copy()
                p["spheres"][1, 3] = 0.0
                p["rgb"][t["ordinary"][::7]] = (0.9, 0.6, 0.3)
                p["rgb"][t["form"] == 5] = (0.2, 0.9, 0.4)
                p["rgb"][t["ground"]] = (0.6, 0.5, 0.4)
                p["sphere_rgb"][:] = ((0.1, 0.9, 0.9), (0.9, 0.9, 0.1))
        elif name == "fold":
            f = folded(t)
            p["tris"][f, 3:6] = p["tris"][f, 6:9]
            p["form"][f] = 3
        elif name == "unfold":
            d = np.nonzero(t["form"] >= 0)[0]
            p["tris"][d, 3:6] = p["tris"][d, 0:3] + np.array([0.0, 6.0, 2.0], F)
            p["tris"][d, 6:9] = p["tris"][d, 6:9] + np.array([5.0, 0.0, 1.0], F)
            p["tris"][t["needle"], 3:6] = (0.0, 40.0, 0.0)
            p["form"][d] = -1
        else:
            raise KeyError(name)
        form_at = np.full(len(t["kinds"]), -1, np.int8)
        form_at[t["at"]] = p["form"]
        p["form_at"] = form_at
        return p
    return qs._once("deg_pose_" + name, make)


def given(orc, name):
    """keywords of rtx.Scene.pose_prims* for the pose: the arrays it changes, the others None (as uploaded)"""
    p = pose(orc, name)
    if name == "prims_all":
        return dict(v0v1v2=p["tris"], spheres=p["spheres"], rgb=p["rgb"], sphere_rgb=p["sphere_rgb"])
    return dict(v0v1v2=p["tris"], spheres=None, rgb=None, sphere_rgb=None)


def posed(orc, samples, name):
    """render() of an oracle scene created with the posed primitives, and `prims`"""
    return qs._once("deg_posed_" + name, lambda: dict(render(orc, samples, pose(orc, name)), prims=pose(orc, name)))


# ---------------------------------------------------------------------------------------------------------- ray sets
def origins_around(rng, centre, r_lo, r_hi, n, above=None):
    u = rng.normal(size=(n, 3))
    u /= np.linalg.norm(u, axis=1)[:, None]
    o = np.asarray(centre) + u * rng.uniform(r_lo, r_hi, size=(n, 1))
    if above is not None:
        o[:, 1] = np.maximum(np.abs(o[:, 1] - above) + above, above + 5.0)
    return o.astype(F)


def search(orc, osc, prims, seed, centre, r_lo, r_hi, above=None, budget=BUDGET):
    """Aims rays from origins around `centre` at points of the C triangles' segments, the triangles in turn.  A try is a
    point pair (origin, target = origin + REACH (point - origin)); its direction fl(target - origin).
    exposed: orc_closest_hit names a C triangle with finite t > 1 in MODE_BVH and MODE_BRUTE, the same prim and t bits, and
    no component of Ray::new's direction is zero.  grazing: both modes agree on something else or a miss.
    -> dict(tries, found = per form exposed among the tries, exposed / grazing = (origins, targets, directions, expected
    records, units, form of the hit or -1), n_disagree = tries on which the two modes differ)"""
    rng = np.random.default_rng(seed)
    c_tris = np.nonzero(np.isin(prims["form"], C_FORMS) & (np.abs(prims["tris"]).max(axis=1) < 1000.0))[0]     # (not the needle)
    form_at = prims["form_at"]
    found = {f: 0 for f in C_FORMS}
    exposed, grazing, n_disagree, tries = [], [], 0, 0
    block = 2000
    while tries < budget:
        o = origins_around(rng, centre, r_lo, r_hi, block, above)
        s = rng.uniform(0.0, 1.0, size=(block, 1))
        for k in range(block):
            if tries >= budget:
                break
            a, b = segment_of(prims["tris"][c_tris[tries % len(c_tris)]])
            p = (a.astype(np.float64) + s[k] * (b.astype(np.float64) - a)).astype(F)
            target = (o[k] + F(REACH) * (p - o[k])).astype(F)
            d = (target - o[k]).astype(F)
            tries += 1
            u = qs.unit(orc, d)
            h = osc.closest_hit(o[k], u)
            g = osc.closest_hit(o[k], u, mode=orc.MODE_BRUTE)
            same = h.hit == g.hit and (not h.hit or (h.tri == g.tri and F(h.t).tobytes() == F(g.t).tobytes()))
            if not same:
                n_disagree += 1
                continue
            is_c = bool(h.hit) and form_at[h.tri] in C_FORMS
            rec = np.zeros(1, qs.HIT_DTYPE)
            rec["prim"] = NO_HIT
            if h.hit:
                rec["prim"][0], rec["t"][0], rec["p_hit"][0] = h.tri, h.t, list(h.p_hit)
            row = (o[k].copy(), target, d, rec[0], u, int(form_at[h.tri]) if h.hit else -1, tries - 1)
            if is_c:
                if np.isfinite(h.t) and h.t > 1.0 and (u != 0).all():
                    found[int(form_at[h.tri])] += 1
                    exposed.append(row)
            elif len(grazing) < N_SET:
                grazing.append(row)
        per = [sum(1 for r in exposed if r[5] == f) for f in C_FORMS]
        if len(exposed) >= N_SET and min(per) >= MIN_PER_CLASS and len(grazing) >= N_SET:
            break

    def chosen():
        """the first N_SET in search order, among them the first MIN_PER_CLASS of every form"""
        must = sorted(i for f in C_FORMS for i in [j for j, r in enumerate(exposed) if r[5] == f][:MIN_PER_CLASS])
        rest = [i for i in range(len(exposed)) if i not in set(must)]
        return sorted(must + rest[:max(0, N_SET - len(must))])

    def packed(rows):
        if not rows:
            return None
        return (np.stack([r[0] for r in rows]), np.stack([r[1] for r in rows]), np.stack([r[2] for r in rows]),
                np.array([r[3] for r in rows], qs.HIT_DTYPE), np.stack([r[4] for r in rows]), np.array([r[5] for r in rows]))
    return dict(tries=tries, found=found, n_exposed=len(exposed), n_disagree=n_disagree,
                exposed=packed([exposed[i] for i in chosen()]), grazing=packed(grazing[:N_SET]))


def mixed_with(orc, osc, exposed, ordinary_o, ordinary_d, seed):
    """the exposed rays scattered among the ordinary ones -> (origins, directions, expected records, place of the exposed)"""
    n, m = len(ordinary_o), len(exposed[0])
    place = np.sort(np.random.default_rng(seed).choice(n + m, m, replace=False))
    rest = np.setdiff1d(np.arange(n + m), place)
    o, d = np.zeros((n + m, 3), F), np.zeros((n + m, 3), F)
    exp = np.zeros(n + m, qs.HIT_DTYPE)
    o[place], d[place], exp[place] = exposed[0], exposed[2], exposed[3]
    o[rest], d[rest] = ordinary_o, ordinary_d
    exp[rest] = qs.oracle_hits(orc, osc, ordinary_o, ordinary_d, qs.HIT_DTYPE)[0]
    return o, d, exp, place


def ray_sets(orc, samples, name):
    """name: "thicket", "fold" (the thicket under that pose: an oracle scene created with the posed vertices) or "soup"
    -> dict(search's result, mixed = (origins, directions, expected, place), prims, osc)"""
    def make():
        if name == "soup":
            prims, osc = soup(orc, samples), soup_frame(orc, samples)["osc"]
            out = search(orc, osc, prims, 41, (0.0, 0.0, -14.0), 18.0, 40.0)
            a = qs.set_a(orc, samples)["trace"]
            oo, od = a[0][:N_ORDINARY], a[1][:N_ORDINARY]
        else:
            prims = thicket(orc) if name == "thicket" else pose(orc, name)
            osc = (thicket_frame(orc, samples) if name == "thicket" else posed(orc, samples, name))["osc"]
            centre = 0.5 * (prims["mesh_lo"] + prims["mesh_hi"])
            out = search(orc, osc, prims, 40 if name == "thicket" else 42, centre, 150.0, 400.0, above=0.0)
            r = qs.bunny(orc, samples)["sets"]["random"]
            oo, od = r[0][:N_ORDINARY], r[1][:N_ORDINARY]
        out.update(prims=prims, osc=osc)
        if out["exposed"] is not None:
            out["mixed"] = mixed_with(orc, osc, out["exposed"], oo, od, 43)
        return out
    return qs._once("deg_rays_" + name, make)


def as_trace(s):
    """a searched set as query_sets' (origins, directions, expected records, None)"""
    return s[0], s[2], s[3], None


def occlusion_pairs(orc, samples, name):
    """the exposed rays' pairs, then the grazing rays' as controls -> dict(pairs = (origins, targets, expected records,
    expected bytes), n_exposed, flips = exposed pairs the oracle scene WITHOUT the degenerates calls not occluded)"""
    def make():
        rs = ray_sets(orc, samples, name)
        e, g = rs["exposed"], rs["grazing"]
        o, t = np.concatenate([e[0], g[0]]), np.concatenate([e[1], g[1]])
        pairs = qs.pair_sets(orc, rs["osc"], o, t)["occlusion"]
        bare = without(rs["prims"], Z_FORMS + C_FORMS)
        if name == "soup":
            osc = soup_scene(orc, samples, bare)
        else:
            osc = oracle_scene(orc, samples, bare)
        free = qs.pair_sets(orc, osc, e[0], e[1])["occlusion"][3]
        osc.close()
        return dict(pairs=pairs, n_exposed=len(e[0]), flips=int(((pairs[3][:len(e[0])] == 1) & (free == 0)).sum()))
    return qs._once("deg_pairs_" + name, make)


# ---------------------------------------------------------------------------------------------------------- shading
def shade_batch(orc, samples, name, key, light=None, count=NB_LIGHT):
    """shade_sets' composition over a ray set (key: "exposed" or "mixed"), one ray per pixel.  A triangle whose
    orc_triangle_new normal is NaN composes as render_pixel has it: |dot(NaN, d)| is NaN, a lit sample adds NaN, an
    occluded one adds 0 (main.rs:207-226) — np_ref's float32 arithmetic carries the NaN through, and orc_color_to_rgb8
    quantises a NaN colour to 0; tests/test_degenerate_sets.py pins this against orc_render_rows_ex."""
    def make():
        rs = ray_sets(orc, samples, name)
        if key == "exposed":
            o, d = rs["exposed"][0], rs["exposed"][2]
        else:
            o, d = rs["mixed"][0], rs["mixed"][1]
        if name == "soup":
            lt, n = qs.SOUP_VIEW["light_tri"], qs.SOUP_VIEW["nb_light_sample"]
        else:
            lt, n = (orc.LIGHT_TRI if light is None else LIGHTS[light]), count
        osc = rs["osc"]
        tb = tables_of(orc, rs["prims"])
        with np.errstate(invalid="ignore"):
            return ss.shade_set(orc, osc, o, d, 1, n, lt, samples, tb)
    return qs._once("deg_shade_%s_%s_%s" % (name, key, light), make)


# ---------------------------------------------------------------------------------------------------------- 1 x 1 frames
def frames(orc, samples_half):
    """N_FRAMES cameras (prune_sets.frame's construction: the eye at a drawn origin, looking at a point of a C triangle's
    segment, a 1 x 1 frame, a constant sample table: the one primary ray goes through the frame's centre) whose primary ray
    the oracle answers with a C triangle in both modes; the first found of a seeded draw, a NaN-normal one (C1 or C2) among
    them if the budget gives one.  -> dict(tried, frames = [dict(camera, ray, exp, form, ref, lin, stats, tri)])"""
    def make():
        prims = thicket(orc)
        osc = oracle_scene(orc, samples_half, prims)
        rng = np.random.default_rng(44)
        c_tris = np.nonzero(np.isin(prims["form"], C_FORMS) & (np.arange(len(prims["form"])) != prims["needle"]))[0]
        centre = 0.5 * (prims["mesh_lo"] + prims["mesh_hi"])
        out, tried, have_nan = [], 0, False
        while tried < FRAME_BUDGET and (len(out) < N_FRAMES or not have_nan):
            o = origins_around(rng, centre, 150.0, 400.0, 1, 0.0)[0]
            a, b = segment_of(prims["tris"][c_tris[tried % len(c_tris)]])
            p = (a.astype(np.float64) + rng.uniform() * (b.astype(np.float64) - a)).astype(F)
            tried += 1
            eye, look = tuple(float(x) for x in o), tuple(float(x) for x in p)
            ro, rd = ps.primary_ray(orc, 1, 1, 0, 0, eye, look, vs.UP, 30.0, samples_half)
            h, g = osc.closest_hit(ro, rd), osc.closest_hit(ro, rd, mode=orc.MODE_BRUTE)
            if not (h.hit and g.hit and h.tri == g.tri and F(h.t).tobytes() == F(g.t).tobytes()):
                continue
            f = int(prims["form_at"][h.tri])
            if f not in C_FORMS or not (np.isfinite(h.t) and h.t > 1.0 and (rd != 0).all()):
                continue
            if len(out) >= N_FRAMES and f == 5:
                continue
            view = ((1, 1), eye, look, 30.0)
            r = render(orc, samples_half, prims, view)
            r["osc"].close()
            exp = np.zeros(1, qs.HIT_DTYPE)
            exp["prim"][0], exp["t"][0], exp["p_hit"][0] = h.tri, h.t, list(h.p_hit)
            out.append(dict(view=view, ray=(ro, rd), exp=exp, form=f, ref=r["frame"], lin=r["lin"], stats=r["stats"], tri=r["tri"]))
            have_nan = have_nan or f in (3, 4)
        return dict(tried=tried, frames=out, osc=osc)
    return qs._once("deg_frames", make)


# ---------------------------------------------------------------------------------------------------------- lights
def lit(orc, samples, name, light):
    """the frame of an oracle scene created with the thicket (name "thicket") or a pose's primitives and the degenerate
    light: (frame, stats)"""
    def make():
        prims = thicket(orc) if name == "thicket" else pose(orc, name)
        r = render(orc, samples, prims, light_tri=LIGHTS[light])
        r["osc"].close()
        return r["frame"], r["stats"]
    return qs._once("deg_lit_%s_%s" % (name, light), make)


# ---------------------------------------------------------------------------------------------------------- the NaN rule
def same_floats(got, want, nan_allowed, what):
    """Two float words compare equal if their bits are equal, or if both are NaN and the expected one belongs to a named
    field (nan_allowed: a mask of `want`'s shape).  The NaN positions are the same on both sides; a NaN where the oracle
    has a number, or a number where it has a NaN, is a failure."""
    got, want = np.ascontiguousarray(got, F), np.ascontiguousarray(want, F)
    assert got.shape == want.shape, what
    gn, wn = np.isnan(got), np.isnan(want)
    assert np.array_equal(gn, wn), "%s: NaN positions differ at %s" % (what, np.argwhere(gn != wn)[:6].tolist())
    allowed = wn & np.broadcast_to(nan_allowed, want.shape)
    bad = (qs.bits(got) != qs.bits(want)) & ~allowed
    assert not bad.any(), "%s: words differ at %s" % (what, np.argwhere(bad)[:6].tolist())


def nan_prims(prims):
    """per Vec position: may this primitive's stored normal be NaN (a Z, C1 or C2 triangle)"""
    return np.isin(prims["form_at"], NAN_FORMS)
