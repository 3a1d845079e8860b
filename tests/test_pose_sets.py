"""The conditions the pose fixtures (tests/pose_sets.py) must meet to test what they are for, asserted with the CPU oracle
alone: no GPU, no librtx.so."""
import numpy as np
import pytest

import pose_sets as ps
import query_sets as qs
import shade_sets as ss
import view_sets as vs
from query_sets import F, NO_HIT


def area2(pose):
    """squared length of cross(e1, e2) per triangle, float32 throughout"""
    t = np.asarray(pose, F).reshape(-1, 3, 3)
    e1, e2 = t[:, 1] - t[:, 0], t[:, 2] - t[:, 0]
    c = np.cross(e1, e2).astype(F)
    return (c * c).sum(axis=1, dtype=F)


def side_rays(orc, samples, v=ps.SIDE):
    (w, h), eye, look_at, distance = v
    o, d, _, _, _ = ss.camera_raw_rays(orc, w, h, eye, look_at, vs.UP, distance, samples, 1)
    return o, d


def test_identity_is_the_scene_and_the_side_view(orc, samples_seeded):
    p = ps.posed(orc, samples_seeded, "identity")
    assert p["pose"].tobytes() == ps.base(orc)[0].tobytes() and p["pose"].shape == (4969, 9)
    assert np.array_equal(p["pose"][ps.GROUND], np.asarray(orc.GROUND_TRI, F))
    assert np.array_equal(p["frame"], vs.bunny_view(orc, samples_seeded, "side")["frame"])
    assert p["frame"].shape == (27, 44, 3)


@pytest.mark.parametrize("name", [n for n in ps.BUNNY_POSES if n != "identity"])
def test_a_pose_changes_at_least_a_hundred_pixels(orc, samples_seeded, name):
    still, moved = ps.posed(orc, samples_seeded, "identity")["frame"], ps.posed(orc, samples_seeded, name)["frame"]
    changed = int((still != moved).any(axis=2).sum())
    print(name, "changes", changed, "of", still.shape[0] * still.shape[1], "pixels")
    assert changed >= 100, (name, changed)


def test_tilt_moves_the_global_triangle_and_turn_does_not(orc, samples_seeded):
    ground = np.asarray(orc.GROUND_TRI, F)
    assert not np.array_equal(ps.bunny_pose(orc, "tilt")[ps.GROUND], ground)
    for name in ("turn", "shift", "squash"):
        assert np.array_equal(ps.bunny_pose(orc, name)[ps.GROUND], ground), name


def test_shift_leaves_the_unposed_root_box(orc, samples_seeded):
    """the mesh's primary hits under `shift` lie outside the box of the unposed mesh — the tree proper's root — so a stream
    that was not refitted would cull them"""
    p = ps.posed(orc, samples_seeded, "shift")
    mesh = ps.base(orc)[0][:ps.GROUND].reshape(-1, 3)
    lo, hi = mesh.min(axis=0), mesh.max(axis=0)
    o, d = side_rays(orc, samples_seeded)
    on_mesh = np.nonzero((p["tri"].reshape(-1) != NO_HIT) & (p["tri"].reshape(-1) < ps.GROUND))[0]
    assert len(on_mesh) >= 100
    outside = 0
    for k in on_mesh:
        h = p["osc"].closest_hit(o[k], qs.unit(orc, d[k]))
        assert h.hit and h.tri == p["tri"].reshape(-1)[k]
        q = np.array(list(h.p_hit), F)
        outside += bool(((q < lo) | (q > hi)).any())
    # The mesh is 152 wide and 118 deep and moves by (120, 0, -80): its new box still overlaps the old one in a corner, and
    # the hits there are inside the old root box.  The hits that are outside it are the ones an unrefitted stream would miss.
    print("shift: %d of %d mesh hits lie outside the unposed root box" % (outside, len(on_mesh)))
    assert outside >= 100 and 2 * outside > len(on_mesh), (outside, len(on_mesh))
    # every triangle leaves its own old box, and the leaf boxes with it: the move exceeds the largest triangle extent
    old = ps.base(orc)[0][:ps.GROUND].reshape(-1, 3, 3)
    assert (old.max(axis=1) - old.min(axis=1)).max() < min(abs(ps.SHIFT[0]), abs(ps.SHIFT[2]))


def test_no_fixture_ray_has_a_zero_component_but_the_hard_ones(orc, samples_seeded):
    for v in (ps.SIDE, ps.TURNTABLE_VIEW):
        assert (side_rays(orc, samples_seeded, v)[1] != 0).all()
    (_, rd, _), (to, tt, _, _) = ps.query_set(orc, samples_seeded, "identity")
    assert (rd != 0).all() and ((tt - to).astype(F) != 0).all()
    assert (ps.TIE_RAYS[1] != 0).all()
    _, hd, exp, twin = ps.hard_rays(orc, samples_seeded, "turn")
    neg_zero = (hd == 0) & np.signbit(hd)
    assert neg_zero.any(axis=1).all() and len(hd) == 71 and len(hd) % 64 != 0
    # the reference's own tree decides these: a -0.0 component rejects at an ancestor box what the +0.0 twin hits
    differ = int((exp["prim"] != twin["prim"]).sum())
    print("hard rays: %d hit, their twins %d, %d differ" % ((exp["prim"] != NO_HIT).sum(), (twin["prim"] != NO_HIT).sum(), differ))
    assert (twin["prim"] < ps.GROUND).sum() >= 20 and differ >= 20


def test_poses_hold_no_zero_area_triangle_and_stay_in_range(orc, samples_seeded):
    poses = {n: ps.bunny_pose(orc, n) for n in ps.BUNNY_POSES}
    poses.update({"turntable %g" % deg: pose for deg, (pose, _) in zip(ps.TURNTABLE_DEGREES, ps.turntable(orc, samples_seeded))})
    for name, pose in poses.items():
        assert pose.dtype == F and pose.shape == (4969, 9), name
        a = area2(pose)
        assert np.isfinite(a).all() and (a > 0).all(), name
        assert np.isfinite(pose).all() and np.abs(pose).max() <= ps.M, name
        assert np.isfinite(ps.tables(orc, samples_seeded, name)["normals"]).all() if name in ps.BUNNY_POSES else True
    assert np.abs(poses["identity"]).max() == ps.M
    assert (area2(ps.TIE_POSE) > 0).all() and np.array_equal(ps.TIE_POSE[0], ps.TIE_POSE[1])


def test_query_sets_hit_the_posed_mesh(orc, samples_seeded):
    for name in ("turn", "tilt"):
        (_, _, exp), (_, _, _, occ) = ps.query_set(orc, samples_seeded, name)
        still = ps.query_set(orc, samples_seeded, "identity")[0][2]
        assert ((exp["prim"] != NO_HIT) & (exp["prim"] < ps.GROUND)).sum() >= 20, name
        assert (exp["prim"] != still["prim"]).sum() >= 20, name
        assert 0 < occ.sum() < len(occ), name


def test_turntable_frames_differ(orc, samples_seeded):
    frames = [f for _, f in ps.turntable(orc, samples_seeded)]
    assert all(f.shape == (16, 24, 3) for f in frames)
    for a in range(4):
        for b in range(a + 1, 4):
            assert (frames[a] != frames[b]).any(axis=2).sum() >= 20, (a, b)
