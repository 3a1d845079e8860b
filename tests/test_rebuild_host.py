"""A pose whose tree is rebuilt, without a GPU: the header, the exports and the bindings, where the rebuild kernels live in
librtx.so, every argument check against the refitting twins', rtx_scene_rebuilt_records — the host statement of what the
rebuild kernels, the sort and the refit make — against numpy restatements of the key, the shape and the fold on the sizes
at which the shape can go wrong, the surface-area cost of the rebuilt stream beside the refitted one, the unchanged ISA of
the existing kernels, and the sanitizer leg of the host statement."""
import ctypes as C
import importlib
import os
import re
import subprocess

import numpy as np
import pytest

import pose_sets as ps
import rebuild_sets as rs
from query_sets import F, H, W, bits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUNNY = os.path.join(ROOT, "models", "big_bunny.obj")
FUNCS = ("rtx_scene_pose_rebuilt", "rtx_scene_pose_rebuilt_device", "rtx_scene_rebuilt_counts", "rtx_scene_rebuilt_records",
         "rtx_scene_rebuilt_aimed", "rtx_debug_pose_rebuilt")
METHODS = ("pose_rebuilt", "pose_rebuilt_device", "rebuilt_counts", "rebuilt_records", "rebuilt_aimed", "debug_pose_rebuilt")
LEAF, SPHERE, MASK = 0x80000000, 0x40000000, 0x3FFFFFFF


@pytest.fixture(scope="module")
def rtx():
    return importlib.import_module("ray-tracer-rust_amd")


@pytest.fixture(scope="module")
def bunny(rtx, samples_seeded):
    with rtx.default_scene([BUNNY], W, H, samples_seeded, reference_tree=rtx.REFTREE_NEVER, tie_rank=None) as s:
        yield s


# ---------------------------------------------------------------------------------------------- header, exports, kernels
def test_header_declares_the_functions_and_the_library_exports_them(rtx):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rtx.h")).read(), flags=re.S)
    for f in FUNCS:
        assert re.search(r"\bint %s\s*\(" % f, hdr), f
    assert re.search(r"#define RTX_ABI_VERSION 3\b", hdr) and rtx.abi_version() == 3      # additions only
    out = subprocess.check_output(["nm", "-D", "--defined-only", rtx.rtx.LIB_PATH], text=True)
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
    assert set(FUNCS) <= exported, set(FUNCS) - exported
    assert set(FUNCS) <= set(rtx.rtx._SIGS)
    rs_text = open(os.path.join(ROOT, "integration", "rtx_ffi.rs")).read()
    block = re.search(r'extern "C" \{(.*?)\n\}', rs_text, re.S).group(1)
    assert set(FUNCS) <= set(re.findall(r"pub fn (\w+)\(", block)), set(FUNCS) - set(re.findall(r"pub fn (\w+)\(", block))
    for m in METHODS:
        assert callable(getattr(rtx.Scene, m)), m
    readme = open(os.path.join(ROOT, "README.md")).read()
    for name in FUNCS + ("rtx_rebuild.hip", "rtx_rebuild.h"):
        assert name in readme, name
    assert re.search(r"^## 19\. ", open(os.path.join(ROOT, "DESIGN.md")).read(), re.M)
    mk = open(os.path.join(ROOT, "ray-tracer-rust_amd", "csrc", "Makefile")).read()
    assert re.search(r"^UNITS\s*:=.*\brtx_rebuild\b", mk, re.M) and "rtx_rebuild.h" in mk   # the library and `make asm`


def test_rebuild_kernels_live_in_their_own_namespace():
    """librtx.so carries exactly two rtxb:: kernels; the pose and plane units' sets are what they were"""
    lib = os.path.join(ROOT, "ray-tracer-rust_amd", "librtx.so")
    blob = open(lib, "rb").read()

    def kernels(ns):
        return set(m.decode() for m in re.findall(rb"_ZN%d%s\d+([a-z0-9_]+_kernel(?:ILb[01]ELb[01]E)?)" % (len(ns), ns.encode()), blob)
                   if not m.startswith(b"__device_stub__"))

    assert kernels("rtxb") == {"key_kernel", "records_kernel"}, kernels("rtxb")
    assert kernels("rtxp") == {"pose_records_kernel", "refit_short_kernel", "refit_long_kernel"}, kernels("rtxp")
    assert kernels("rtxg") == {"global_planes_kernel"}, kernels("rtxg")
    symbols = subprocess.run(["nm", "-C", lib], capture_output=True, text=True, check=True).stdout
    host_side = set(k for k in re.findall(r"\brtxb::(\w+_kernel)\(", symbols) if not k.startswith("__device_stub__"))
    assert host_side == {"key_kernel", "records_kernel"}, host_side
    undefined = subprocess.run(["nm", "-D", "--undefined-only", lib], capture_output=True, text=True, check=True).stdout
    assert "getenv" not in undefined                                 # (the unit instantiates rocprim, as rtx_query does)


def test_existing_kernels_are_unchanged():
    """profiles/pose_rebuild_same_isa.txt: tools/same_isa.py over `make asm` of the parent commit and of this one, every
    existing unit — one SAME line per kernel and no other verdict"""
    text = open(os.path.join(ROOT, "profiles", "pose_rebuild_same_isa.txt")).read()
    verdicts = re.findall(r"^\s*(SAME|DIFF|MISSING)\b", text, re.M)
    assert len(verdicts) >= 20 and set(verdicts) == {"SAME"}, text
    for unit in ("rtx_kernel", "rtx_query", "rtx_shade", "rtx_view", "rtx_aim", "rtx_light", "rtx_tour", "rtx_pose", "rtx_planes"):
        assert unit + ".gfx950.s" in text, unit


# ---------------------------------------------------------------------------------------------- argument checks
def test_argument_checks_are_the_twins_and_need_no_device(rtx, orc, bunny):
    L = rtx.rtx._lib
    h = bunny.handle
    BAD, UNSUPPORTED, NO_DEVICE, OK = rtx.ERR_BAD_ARG, rtx.ERR_UNSUPPORTED, rtx.ERR_NO_DEVICE, rtx.OK
    u32p, f32p = rtx.rtx.u32p, rtx.rtx.f32p
    pose = ps.bunny_pose(orc, "turn")
    vp = pose.ctypes.data_as(f32p)
    rank = np.arange(4969, dtype=np.uint32)

    def both(expected, *args):
        got = L.rtx_scene_pose_rebuilt(*args), L.rtx_scene_pose(*args)
        assert got == (expected, expected), (got, expected)

    both(BAD, None, 99, vp, None, rtx.REFTREE_NEVER, None)
    both(BAD, h, 99, None, None, rtx.REFTREE_NEVER, None)
    both(BAD, h, 99, vp, None, 3, None)
    both(NO_DEVICE, h, 99, vp, None, rtx.REFTREE_NEVER, None)
    both(NO_DEVICE, h, -1, vp, rank.ctypes.data_as(u32p), rtx.REFTREE_NEVER, None)
    # the range rule and non-finite vertices, decided before a device is looked for
    for where, value in ((0, np.nan), (17, np.inf), (4968 * 9 + 8, -np.inf), (100, 10000.001), (4968 * 9, -10001.0)):
        bad = pose.copy()
        bad.reshape(-1)[where] = value
        both(UNSUPPORTED, h, 99, bad.ctypes.data_as(f32p), None, rtx.REFTREE_NEVER, None)
    edge = pose.copy()
    edge.reshape(-1)[5] = -10000.0                        # at the bound: in range
    both(NO_DEVICE, h, 99, edge.ctypes.data_as(f32p), None, rtx.REFTREE_NEVER, None)

    def both_device(expected, *args):
        got = L.rtx_scene_pose_rebuilt_device(*args), L.rtx_scene_pose_device(*args)
        assert got == (expected, expected), (got, expected)

    both_device(BAD, None, 99, 256, None, None)
    both_device(BAD, h, 99, None, None, None)
    both_device(BAD, h, 99, 258, None, None)
    both_device(BAD, h, 99, 256, 513, None)
    both_device(NO_DEVICE, h, 99, 256, None, None)
    both_device(NO_DEVICE, h, 99, 256, 512, None)
    # the readers
    n = C.c_uint32(0)
    assert L.rtx_scene_rebuilt_counts(None, C.byref(n)) == BAD and L.rtx_scene_rebuilt_counts(h, None) == BAD
    assert L.rtx_scene_rebuilt_counts(h, C.byref(n)) == OK and n.value == bunny.rebuilt_counts() > 0
    assert L.rtx_scene_rebuilt_records(None, vp, None, None, None, None, None, None) == BAD
    assert L.rtx_scene_rebuilt_records(h, None, None, None, None, None, None, None) == BAD
    assert L.rtx_scene_rebuilt_records(h, vp, None, None, None, None, None, None) == OK      # every output may be NULL
    eye = np.zeros(3, F).ctypes.data_as(f32p)
    aimed = np.zeros((n.value, 8), np.uint32).ctypes.data_as(u32p)
    assert L.rtx_scene_rebuilt_aimed(None, vp, eye, aimed) == BAD and L.rtx_scene_rebuilt_aimed(h, None, eye, aimed) == BAD
    assert L.rtx_scene_rebuilt_aimed(h, vp, None, aimed) == BAD and L.rtx_scene_rebuilt_aimed(h, vp, eye, None) == BAD
    assert L.rtx_scene_rebuilt_aimed(h, vp, eye, aimed) == OK
    assert L.rtx_debug_pose_rebuilt(None, 99, None, None, None, None, None, None) == BAD
    assert L.rtx_debug_pose_rebuilt(h, 99, None, None, None, None, None, aimed) == BAD       # out_aimed without an eye
    assert L.rtx_debug_pose_rebuilt(h, 99, eye, None, None, None, None, aimed) == NO_DEVICE
    assert L.rtx_debug_pose_rebuilt(h, 99, None, None, None, None, None, None) == NO_DEVICE


# ---------------------------------------------------------------------------------------------- the host statement
def kinds_of(scene):
    if scene.kinds is not None:
        return np.asarray(scene.kinds, np.uint8)
    n_sph = 0 if scene.spheres is None else len(scene.spheres)
    return np.concatenate([np.zeros(len(scene.tris), np.uint8), np.ones(n_sph, np.uint8)])


def check_statement(rtx, scene, pose, name, leaf_max=rs.LEAF_MAX, tie_rank=None):
    """rtx_scene_rebuilt_records of `pose` against numpy: the permutation, the keys, the records, the shape and the boxes"""
    n, ng = scene.n_prims, scene.info()["n_global"]
    keys, perm, t, s, nodes = scene.rebuilt_records(pose, tie_rank=tie_rank)
    pt, pshade, _ = scene.posed_records(pose, tie_rank=tie_rank)            # the same pose's records in uploaded order
    # the permutation: of the tree proper; keys rise along it, equal keys keep uploaded order
    assert np.array_equal(np.sort(perm), np.arange(ng, n)), name
    assert (keys[1:] >= keys[:-1]).all(), name
    equal = keys[1:] == keys[:-1]
    assert (perm[1:][equal] > perm[:-1][equal]).all(), name
    # the records: the global triangles' in place, then the posed records in sorted order; shading as any pose's
    assert np.array_equal(t[:ng], pt[:ng]) and np.array_equal(t[ng:], pt[perm]), name
    assert np.array_equal(s, pshade), name
    sphere = kinds_of(scene)[t[:, 15]] != 0
    assert not sphere[:ng].any(), name
    n_sph = int(sphere.sum())
    assert not sphere[:n - n_sph].any() and sphere[n - n_sph:].all(), name + ": spheres sort behind the triangles"
    # the keys, restated
    want = rs.numpy_keys(t[ng:], sphere[ng:], scene.pose_bound())
    assert np.array_equal(keys, want), (name, np.nonzero(keys != want)[0][:5])
    # the shape: a closed form of the counts
    link, info, runs = rs.shape(ng, n - ng - n_sph, n_sph, leaf_max)
    assert len(nodes) == len(link) == scene.rebuilt_counts(), (name, len(nodes), len(link))
    assert np.array_equal(nodes[:, 3], link) and np.array_equal(nodes[:, 7], info), name
    check_shape(nodes, ng, n, leaf_max, sphere, name)
    assert np.array_equal(ps.node_ranges(nodes), runs), name
    # the boxes: the fold of the records' own boxes over every node's run, moved by cull_delta
    fold = ps.numpy_fold(t, nodes, ps.cull_delta(scene.pose_bound()))
    assert np.array_equal(bits(nodes.view(F)[:, 0:3]), bits(fold[:, :3])) and np.array_equal(bits(nodes.view(F)[:, 4:7]), bits(fold[:, 3:])), name
    # the aimed stream for an eye: the same records in another pre-order (a scene that aims nothing: the same words)
    aimed = scene.rebuilt_aimed(pose, (30.0, 120.0, 250.0))
    if scene.primary_nodes()[1]:
        root = 2 if (ng and len(nodes) > 2) else 0
        assert np.array_equal(aimed[:root, [0, 1, 2, 4, 5, 6, 7]], nodes[:root, [0, 1, 2, 4, 5, 6, 7]]), name
        boxes = lambda a: sorted(map(bytes, np.ascontiguousarray(a[root:, [0, 1, 2, 4, 5, 6]])))
        assert boxes(aimed) == boxes(nodes), name
        check_shape(aimed, ng, n, leaf_max, sphere, name + " aimed", in_order=False)
    else:
        assert np.array_equal(aimed, nodes), name
    return keys, perm, t, s, nodes


def check_shape(nodes, ng, n, leaf_max, sphere, name, in_order=True):
    """the stream from its words alone: pre-order links, runs that concatenate, leaves of one arm and at most leaf_max
    records, every record of the tree proper in exactly one leaf, the root and the global leaf where a created scene's are"""
    info, link = nodes[:, 7].astype(np.int64), nodes[:, 3].astype(np.int64)
    leaf = (info & LEAF) != 0
    nn = len(nodes)
    runs = ps.node_ranges(nodes)             # (in_order: the first child's run comes first; an aimed stream may swap them)
    covered = np.zeros(n, np.int64)
    for i in range(nn):
        if leaf[i]:
            first, count = info[i] & MASK, link[i]
            covered[first:first + count] += 1
            if ng and i == (1 if nn > 1 else 0):
                assert (first, count) == (0, ng) and not (info[i] & SPHERE), name          # the global leaf
                continue
            assert 1 <= count <= leaf_max, (name, i, count)
            arm = sphere[first:first + count]
            assert (arm == arm[0]).all() and bool(info[i] & SPHERE) == bool(arm[0]), (name, i)
        else:
            a, b = i + 1, info[i]
            end_a = a + 1 if leaf[a] else link[a]
            end_b = b + 1 if leaf[b] else link[b]
            assert b == end_a and link[i] == end_b and i < a < b < link[i] <= nn, (name, i)
            if not in_order and runs[b][0] < runs[a][0]:
                a, b = b, a
            assert runs[a][0] == runs[i][0] and runs[a][0] + runs[a][1] == runs[b][0], (name, i)
            assert runs[b][0] + runs[b][1] == runs[i][0] + runs[i][1], (name, i)
    assert (covered == 1).all(), name
    if ng and nn > 1:
        assert not leaf[0] and info[0] == 2 and link[0] == nn and tuple(runs[0]) == (0, n), name


def test_the_statement_on_the_sizes_at_which_the_shape_can_go_wrong(rtx, samples_seeded):
    seen = {False: set(), True: set()}      # sizes of the tree proper, without and with global triangles
    for name, sc in rs.shape_scenes(rtx).items():
        with ps.open_small(rtx, samples_seeded, sc) as scene:
            ng, n = scene.info()["n_global"], scene.n_prims
            if "ground" in name:
                assert ng == 1, name
            seen[ng != 0].add(n - ng)
            own = np.ascontiguousarray(scene.tris.copy())
            # the identity pose: the uploaded records as a multiset, every idx's words equal
            keys, perm, t, s, nodes = check_statement(rtx, scene, own, name + " identity")
            up = scene.posed_records(own)[0]
            assert np.array_equal(t[np.argsort(t[:, 15])], up[np.argsort(up[:, 15])]), name
            check_statement(rtx, scene, sc[4], name, tie_rank=np.arange(n, dtype=np.uint32)[::-1].copy())
            created, _ = scene.nodes()
            if ng and n > ng:        # root, global leaf, tree proper: laid out as the created scene's are
                assert np.array_equal(nodes[:2, 7], created[:2, 7]) and nodes[1, 3] == created[1, 3] == ng, name
                assert nodes[0, 3] == len(nodes) and created[0, 3] == len(created), name
            if "coincident" in name:
                assert (keys[1:] == keys[:-1]).sum() >= 5, name                           # the fixture does hold equal keys
    lm, lane = rs.LEAF_MAX, rtx.rtx.POSE_LANE_MAX
    sizes = {2, lm, lm + 1, 2 * lm + 1, lane, lane + 1, 255, 256, 257}
    assert sizes <= seen[False] and sizes | {0, 1} <= seen[True], seen      # (a triangle alone is its scene's global one)


def test_another_leaf_max_and_spheres_only(rtx, samples_seeded):
    sc = rs.shape_scenes(rtx)["soup257_ground"]
    for leaf_max in (1, 7):
        with ps.open_small(rtx, samples_seeded, sc, leaf_max=leaf_max) as scene:
            check_statement(rtx, scene, sc[4], "leaf_max %d" % leaf_max, leaf_max=leaf_max)
    rng = np.random.default_rng(22)
    spheres = np.concatenate([rng.uniform(-40, 40, (13, 3)), rng.uniform(0.5, 3.0, (13, 1))], axis=1).astype(F)
    only = (np.zeros((0, 9), F), spheres, np.ones(13, np.uint8), {}, np.zeros((0, 9), F))
    with ps.open_small(rtx, samples_seeded, only) as scene:
        keys, perm, t, s, nodes = check_statement(rtx, scene, only[4], "spheres only")
        assert (keys >> np.uint64(63) == 1).all() and (nodes[(nodes[:, 7] & LEAF) != 0, 7] & SPHERE).all()


def test_twenty_thousand_triangles(rtx, samples_seeded):
    soup, redrawn = rtx.synthetic_mesh(20000), rtx.synthetic_mesh(20000, seed=rs.SCATTER_SEED)
    with ps.open_small(rtx, samples_seeded, (soup, None, None, {}, redrawn)) as scene:
        check_statement(rtx, scene, redrawn, "soup20000")


def test_bunny_poses_on_the_host(rtx, orc, bunny):
    for name in ps.BUNNY_POSES:
        check_statement(rtx, bunny, ps.bunny_pose(orc, name), name)


# ---------------------------------------------------------------------------------------------- tree quality
def test_surface_area_cost_rebuilt_against_refitted(rtx, orc, samples_seeded, bunny, capsys):
    """The surface-area cost (rebuild_sets.sah_cost) of the rebuilt stream and of the refitted one.  Asserted: for the
    scatter pose — the case DESIGN section 17 names — the rebuilt tree costs less.  Recorded in DESIGN section 19:
    scatter 197.1 rebuilt against 7,860.1 refitted (the created tree over the unposed soup: 71.4); big_bunny's 40-degree turn
    72.3 rebuilt against 30.7 refitted — the rigid turn favours the refit."""
    tris, pose = rs.scatter(rtx)
    with rs.scatter_scene(rtx, samples_seeded) as scene:
        ng = scene.info()["n_global"]
        assert ng == 1
        rebuilt = rs.sah_cost(scene.rebuilt_records(pose)[4], ng)
        refitted = rs.sah_cost(scene.posed_records(pose)[2], ng)
        created = rs.sah_cost(scene.posed_records(tris)[2], ng)
    turn = ps.bunny_pose(orc, "turn")
    t_rebuilt = rs.sah_cost(bunny.rebuilt_records(turn)[4], 1)
    t_refitted = rs.sah_cost(bunny.posed_records(turn)[2], 1)
    with capsys.disabled():
        print("\nsurface-area cost: scatter rebuilt %.1f refitted %.1f (created, unposed %.1f); turn rebuilt %.1f refitted %.1f"
              % (rebuilt, refitted, created, t_rebuilt, t_refitted))
    assert rebuilt < refitted, (rebuilt, refitted)


# ---------------------------------------------------------------------------------------------- sanitizers
def test_host_statement_is_clean_under_asan_and_ubsan(tmp_path):
    out = subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "tests", "sanitize_rebuild"), "run", "OUT=%s" % tmp_path],
                         capture_output=True, text=True, timeout=900)
    text = out.stdout + out.stderr
    assert out.returncode == 0, text[-4000:]
    assert "rebuild sanitizer driver: 0 failed checks" in text
    assert "ERROR: AddressSanitizer" not in text and "runtime error" not in text and "LeakSanitizer" not in text, text[-4000:]
