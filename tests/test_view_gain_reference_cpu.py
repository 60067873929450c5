"""tests/view_gain_reference.py, the numpy restatement of the next-best-view entry points, held to what the feature is FOR on
volumes with known answers: what a wall hides and from where, what ``max_unknown`` and an interest mask do to one ray, the
greedy joint order on a planted plane, and a box seen from one side.  No GPU.

The hand-set volumes are dyadic (voxel 1/8, origin on the lattice), so every ray point is exact in float32 and the sets below
are enumerated by hand.
"""
import functools

import numpy as np

from . import approach_volume_reference as href
from . import tsdf_raycast_reference as ray
from . import view_gain_reference as vg
from .icp_projective_reference import look_at, rectangle, render

f32 = np.float32
BEHIND = np.array([[-1.0, 0, 0, 0], [0, 1.0, 0, 0], [0, 0, -1.0, 1.25], [0, 0, 0, 1.0]])     # at z = 1.25, looking along -z
FRONT = np.array([[1.0, 0, 0, 0], [0, 1.0, 0, 0], [0, 0, 1.0, -0.25], [0, 0, 0, 1.0]])       # at z = -0.25, looking along +z
K16 = (16.0, 16.0, 1.5, 1.5)             # 4 x 4 pixels, du = -1.5 .. 1.5: |x| <= 1.5 * 0.6875 / 16 < 1/8, never 0


def wall_volume():
    """8^3 voxels of 1/8 over [-0.5, 0.5)^2 x [0, 1): FREE for iz 0..2, a SOLID wall at iz 3, never observed behind it."""
    hand = href.HandVolume((8, 8, 8), (-0.5, -0.5, 0.0), 0.125, trunc=0.5)
    iz = np.arange(hand.D.shape[0]) // 64
    hand.W[iz <= 3] = 1
    hand.D[iz == 3] = -0.5
    return hand


def _mark(hand, poses, k, size, near, step, n_steps, max_unknown, interest=None, margin=0.0):
    return vg.view_mark(vg.Planes.of(hand), margin, k, np.asarray(poses), size[0], size[1], near, step, n_steps, max_unknown, interest)


def test_a_wall_hides_what_is_behind_it_from_the_front_and_not_from_behind():
    hand = wall_volume()
    # samples at camera depth 0.3125 + 0.125 i: the voxel centres of the eight layers, from either side
    out = _mark(hand, [FRONT, BEHIND], K16, (4, 4), 0.3125, 0.125, 8, 8)
    assert out["sets"][0] == set() and (out["status"][0] == vg.BLOCKED).all() and out["rays"][0].tolist() == [0, 16, 0, 0]
    # from behind: the rays stay within |x|, |y| < 1/8 of the axis, so they cross ix, iy in {3, 4}, and iz 7, 6, 5, 4 before the wall
    by_hand = {hand.at(ix, iy, iz) for ix in (3, 4) for iy in (3, 4) for iz in (4, 5, 6, 7)}
    assert out["sets"][1] == by_hand and (out["status"][1] == vg.BLOCKED).all() and out["rays"][1].tolist() == [0, 16, 0, 16]
    assert set(np.nonzero(out["plane"])[0].tolist()) == by_hand and (out["plane"][sorted(by_hand)] == 2).all()
    # the wall one ulp either side of d_solid (margin / trunc = 0.25): at and above it the wall is FREE and the rays pass
    for d, blocked in ((np.nextafter(f32(0.25), f32(-1)), True), (f32(0.25), False), (np.nextafter(f32(0.25), f32(1)), False)):
        hand.D[np.arange(512) // 64 == 3] = d
        got = _mark(hand, [FRONT], K16, (4, 4), 0.3125, 0.125, 8, 8, margin=0.125)
        assert (got["status"][0] == (vg.BLOCKED if blocked else vg.EXITED)).all() and (len(got["sets"][0]) == 0) == blocked


ON_AXIS = (8.0, 8.0, 0.0, 0.0)           # one pixel, its ray the camera's axis: x = y = 0, the face between ix, iy 3 and 4 -> 4


def test_max_unknown_counts_samples_and_an_interest_mask_restricts_marks_not_saturation():
    slab = href.HandVolume((8, 8, 8), (-0.5, -0.5, 0.0), 0.125, trunc=0.5)          # never observed anywhere
    column = [slab.at(4, 4, iz) for iz in range(8)]
    # two samples per voxel: camera depth 0.28125 + 0.0625 i -> z = 0.03125 + 0.0625 i, layers 0, 0, 1, 1, 2, 2, ...
    for m, layers in ((1, 1), (3, 2), (5, 3), (16, 8)):
        out = _mark(slab, [FRONT], ON_AXIS, (1, 1), 0.28125, 0.0625, 16, m)
        assert out["sets"][0] == set(column[:layers]), m
        assert out["status"].tolist() == [[vg.SATURATED]] and out["rays"].tolist() == [[0, 0, 1, 1]], m
    # a ray that leaves the slab before it has counted max_unknown samples EXITED
    slab.W[np.arange(512) // 64 >= 2] = 1                                           # seen free beyond layer 1
    out = _mark(slab, [FRONT], ON_AXIS, (1, 1), 0.28125, 0.0625, 16, 5)
    assert out["sets"][0] == set(column[:2]) and out["status"].tolist() == [[vg.EXITED]] and out["rays"].tolist() == [[1, 0, 0, 1]]
    slab.W[:] = 0
    for wanted, marks in ((2, [2]), (5, []), (0, [0])):
        interest = np.zeros((512,), dtype=np.uint8)
        interest[column[wanted]] = 1
        out = _mark(slab, [FRONT], ON_AXIS, (1, 1), 0.28125, 0.0625, 16, 5, interest)
        assert out["sets"][0] == {column[j] for j in marks}, wanted
        assert out["status"].tolist() == [[vg.SATURATED]] and out["rays"].tolist() == [[0, 0, 1, 1 if marks else 0]], wanted
    out = _mark(slab, [FRONT], ON_AXIS, (1, 1), 0.28125, 0.0625, 16, 5, np.zeros((512,), dtype=np.uint8))
    assert not out["plane"].any() and out["rays"].tolist() == [[0, 0, 1, 0]]


def planted_plane(n=300):
    """Poses 0 and 1 see the same ten words, pose 2 four others, pose 3 two of pose 2's and one of its own -> (plane, P)."""
    plane = np.zeros((n,), dtype=np.uint32)
    plane[10:20] |= 0b0011
    plane[100:104] |= 0b0100
    plane[102:104] |= 0b1000
    plane[n - 1] |= 0b1000
    return plane, 4


def test_the_greedy_order_is_joint_ties_go_to_the_lowest_index_and_min_gain_ends_it():
    plane, P = planted_plane()
    sets = vg.plane_sets(plane, P)
    gain, order, order_gain = vg.view_pick(sets, 4)
    assert gain.tolist() == [10, 10, 4, 3]                       # by single gain the order would be 0, 1, 2, 3
    assert order.tolist() == [0, 2, 3, -1] and order_gain.tolist() == [10, 4, 1, 0]      # pose 1 adds nothing to pose 0
    assert [a.dtype for a in (gain, order, order_gain)] == [np.int32] * 3
    assert vg.view_pick(sets, 1)[1].tolist() == [0]              # the tie of poses 0 and 1
    assert vg.view_pick(sets[::-1], 2)[1].tolist() == [2, 1]     # reversed: poses 2 and 3 tie at ten, 2 wins; then old pose 2
    gain, order, order_gain = vg.view_pick(sets, 4, min_gain=4)
    assert order.tolist() == [0, 2, -1, -1] and order_gain.tolist() == [10, 4, 0, 0]
    assert vg.view_pick(sets, 3, min_gain=11)[1].tolist() == [-1, -1, -1]
    assert vg.view_pick([set(), set()], 2)[1].tolist() == [-1, -1]                       # max(min_gain, 1): nothing to gain


# ---- a box seen from one side ---------------------------------------------------------------------------------------------------
def _box(lo, hi):
    lo, hi = np.asarray(lo, dtype=np.float64), np.asarray(hi, dtype=np.float64)
    e = np.diag(hi - lo)
    return ([rectangle(lo, e[a], e[b]) for a, b in ((0, 1), (0, 2), (1, 2))]
            + [rectangle(hi, -e[a], -e[b]) for a, b in ((0, 1), (0, 2), (1, 2))])


BOX_SCENE = _box((-0.08, -0.03, 0.47), (0.08, 0.03, 0.53)) + [rectangle((-2, -2, 0.7), (4, 0, 0), (0, 4, 0))]      # and a far wall
BOX_VOLUME = dict(voxel=0.01, trunc=0.03, origin=(-0.16, -0.16, 0.34), dims=(32, 32, 28), max_points=1 << 14)
BOX_CAMERA = (64, 48, (50.0, 50.0, 31.5, 23.5))
BOX_TARGET = np.array([0.0, 0.0, 0.5])
ORBIT = [(az, el) for el in (0, 40) for az in range(0, 360, 45)]          # azimuth 0, elevation 0: the first camera's own pose
VIRTUAL = dict(intrinsics=(40.0, 40.0, 19.5, 14.5), width=40, height=30, near=0.1, step=0.01, n_steps=80, max_unknown=5)
GRASP_L = href.rows_of(np.array([[[0.0, 0, 1], [1, 0, 0], [0, 1, 0]]]), np.array([[0.06, -0.05, 0.5]]))
GRASP_BOX = href.gripper_box(0.06, 0.08)


def orbit_pose(azimuth, elevation, radius=0.5):
    a, e = np.radians(azimuth), np.radians(elevation)
    eye = BOX_TARGET + radius * np.array([np.cos(e) * np.sin(a), -np.sin(e), -np.cos(e) * np.cos(a)])
    return look_at(eye, BOX_TARGET, up=(0.0, -1.0, 0.0))


@functools.lru_cache(maxsize=None)
def box_scene():
    """The box integrated from the identity view -> (the restated volume, its ``Planes``, the 16 orbit poses (16,4,4))."""
    width, height, k = BOX_CAMERA
    vol = ray.Volume(**BOX_VOLUME)
    vol.integrate(render(BOX_SCENE, width, height, k), None, width, height, k)
    return vol, vg.Planes.of(vol), np.stack([orbit_pose(*angles) for angles in ORBIT])


def test_a_box_from_one_view_ranks_the_far_side_first_and_the_view_it_has_last():
    """What one view of a box leaves unobserved is its inside and its shadow.  The first camera's own pose sees none of it: its
    rays end on the surface it has seen.  The far side looks straight into the 16 cm wide shadow; a side view into its 6 cm end.
    The gains the restatement gives (DESIGN.md par. 5): own pose 0; azimuth 180 at elevation 0 / 40: 796 / 807; the best pose
    off the far side, azimuth 135 at 40: 677."""
    _, planes, poses = box_scene()
    out = vg.view_mark(planes, 0.0, poses=poses, **VIRTUAL)
    gain, order, order_gain = vg.view_pick(out["sets"], 4)
    print("gain per (azimuth, elevation):", dict(zip(ORBIT, gain.tolist())), "order", order.tolist(), order_gain.tolist())
    assert np.allclose(poses[0], np.eye(4), atol=1e-12)
    assert gain[0] == 0 and (gain[1:] > 0).all() and (out["status"][0] != vg.SATURATED).all()       # the view it already has: last
    ranked = np.argsort(-gain, kind="stable")
    assert {ORBIT[j][0] for j in ranked[:2]} == {180}                                               # the far side: first
    assert gain[ranked[0]] >= 1.15 * max(g for j, g in enumerate(gain) if ORBIT[j][0] != 180)       # ... with room to spare
    assert order[0] == ranked[0] and order_gain[0] == gain[ranked[0]] and (np.diff(order_gain) <= 0).all()
    assert len(set(order.tolist())) == 4 and order_gain[1] < gain[order[1]]                         # the second pick is joint


def test_with_the_interest_of_a_grasp_the_winner_sees_its_far_finger_lane():
    """A grasp from above near the box's +x end, closing along the first camera's axis, its hand one voxel thick: the near finger
    is in seen free space; unobserved are the box's inside between the fingers, beyond the band the first view measured (z >= 0.50),
    and the far finger's lane behind the box (z in 0.54 .. 0.55), 20 voxels in all.  The far side's rays saturate before they
    reach them (7 cm of shadow lie between); from the +x side they are 2 cm in.  Restated gains over the 20 voxels: azimuth 90 at
    elevation 0: 20; far side at 0: 0."""
    _, planes, poses = box_scene()
    interest, counts = vg.interest_hands(planes, 0.0, GRASP_L, GRASP_BOX, 0.05, 0.01, 0.06)
    lane = np.nonzero(interest)[0]
    assert counts.tolist() == [20] and len(lane) == 20 and (lane // (32 * 32) >= 16).all() and (lane // (32 * 32) == 20).sum() == 4   # z >= 0.50; the far finger's lane
    out = vg.view_mark(planes, 0.0, poses=poses, interest=interest, **VIRTUAL)
    gain, order, order_gain = vg.view_pick(out["sets"], 2)
    print("lane gain per (azimuth, elevation):", dict(zip(ORBIT, gain.tolist())))
    assert ORBIT[order[0]] == (90, 0) and out["sets"][order[0]] == set(lane.tolist()) and order_gain.tolist() == [20, 0]
    assert order[1] == -1 and gain[0] == 0 and gain[ORBIT.index((180, 0))] == 0
    assert all(s <= set(lane.tolist()) for s in out["sets"])                                        # nothing else is marked
    free = vg.view_mark(planes, 0.0, poses=poses, **VIRTUAL)
    assert (free["status"] == out["status"]).all()                                                  # the mask moves no ray's end
