"""tests/approach_volume_reference.py, the numpy restatement of the approach analysis against the TSDF volume, held to things it
can be wrong about: what one view of a box leaves unseen behind it and what a second view from the other side adds, the closing
width of the fused box, the clearance in front of a rendered wall, one hand-built volume per classification rule, and the host
side of the feature (parameters, lattice counts, CLI flags, the header's prototype).  No GPU.

The volume is tests/tsdf_reference.py's, the views are tests/icp_projective_reference.py's analytic renderer.
"""
import ctypes

import numpy as np
import pytest

from . import approach_volume_reference as ref
from . import tsdf_reference as tsdf_ref
from .icp_projective_reference import look_at, rectangle, render

f32 = np.float32
inf = float("inf")
W, H = 256, 192
K = (240.0, 240.0, 127.5, 95.5)              # a pixel is under 2 mm wide at 0.45 m: less than half the 5 mm voxel
VOXEL = 0.005
SMALL = dict(voxel=VOXEL, trunc=0.01, origin=(-0.12, -0.10, -0.015), dims=(48, 40, 36), max_points=1 << 14)
WIDTH, DEPTH = 0.08, 0.06
GRIPPER = ref.gripper_box(DEPTH, WIDTH)      # x_lo -0.06, x_hi 0.06, ht 0.005, hw 0.05, hs 0.04, back_x -0.0
BOX_HALF_Y, BOX_HALF_X, BOX_TOP = 0.03, 0.03, 0.06
CAMERAS = [look_at((0.0, -0.35, 0.30), (0.0, 0.0, 0.03)), look_at((0.0, 0.35, 0.30), (0.0, 0.0, 0.03))]
TOP_DOWN = np.array([[0.0, 0.0, 1.0], [0.0, 1.0, 0.0], [-1.0, 0.0, 0.0]])   # columns: approach -z, closing +y, minor +x


def box_on_table():
    x, y, t = BOX_HALF_X, BOX_HALF_Y, BOX_TOP
    return [rectangle((-0.5, -0.5, 0.0), (1.0, 0, 0), (0, 1.0, 0)),                    # the table, z = 0
            rectangle((-x, -y, t), (2 * x, 0, 0), (0, 2 * y, 0)),                      # the box's top
            rectangle((-x, -y, 0.0), (2 * x, 0, 0), (0, 0, t)), rectangle((-x, y, 0.0), (2 * x, 0, 0), (0, 0, t)),   # y = -+0.03
            rectangle((-x, -y, 0.0), (0, 2 * y, 0), (0, 0, t)), rectangle((x, -y, 0.0), (0, 2 * y, 0), (0, 0, t))]   # x = -+0.03


@pytest.fixture(scope="module")
def fused():
    """The box seen from the -y side, then also from the +y side -> (volume after one view as (D, W), after two)."""
    scene = box_on_table()
    vol = tsdf_ref.Volume(**SMALL)
    states = []
    for pose in CAMERAS:
        counts = vol.integrate(render(scene, W, H, K, pose), None, W, H, K, pose)
        assert counts[tsdf_ref.UPDATED] > 10000
        states.append((vol.D.copy(), vol.W.copy()))
    return vol, states


def _run(vol, state, L, standoff=0.02, step=VOXEL, margin=0.0, box=GRIPPER, x_extent=DEPTH):
    D, Wt = state
    return ref.approach_volume_ref(D, Wt, vol.dims, vol.origin, vol.p["voxel"], vol.p["trunc"], vol.p["min_weight"], margin, L, box,
                                   standoff, step, x_extent)


def test_one_view_leaves_the_far_finger_lane_unseen_and_a_second_view_fills_it(fused):
    """A top-down grasp 8 cm above the table, closing along y over the 6 cm box: the fingers go down at |y| in (4, 5) cm, in front
    of the box for the first camera (y < 0) and behind it (y > 0), where its rays end on the box's top and front."""
    vol, (one, two) = fused
    L = ref.rows_of(TOP_DOWN[None], [[0.0, 0.0, 0.08]])
    xv, yv, zv = ref.lattice_samples(GRIPPER, 0.02, VOXEL, DEPTH)
    x, y, z = xv[:, None, None], yv[None, :, None], zv[None, None, :]
    lane = (x > 0.02) & (x < f32(DEPTH)) & (np.abs(z) < f32(0.005))        # the lower 4 cm of a finger: world z in (2, 6) cm
    far, near = lane & (y > f32(0.04)) & (y < f32(0.05)), lane & (y < f32(-0.04)) & (y > f32(-0.05))
    shares = []
    for state in (one, two):
        _, _, unseen = ref.classify(state[0], state[1], vol.dims, vol.origin, VOXEL, 1, f32(0.0), L[0], x, y, z)
        shares.append((unseen[np.broadcast_to(far, unseen.shape)].mean(), unseen[np.broadcast_to(near, unseen.shape)].mean()))
    print("unseen share of the far / near finger lane: one view %.2f / %.2f, two views %.2f / %.2f" % (shares[0] + shares[1]))
    assert shares[0][0] > 0.5 and shares[0][1] == 0.0                       # behind the box: mostly unseen; in front: seen free
    assert shares[1][0] == 0.0 and shares[1][1] == 0.0                      # the second camera looks into the far lane

    (c1, v1), (c2, v2) = _run(vol, one, L), _run(vol, two, L)
    d1 = ref.derived_ref(c1, v1, TOP_DOWN[None], [[0.0, 0.0, 0.08]], 0.005, GRIPPER[4])
    d2 = ref.derived_ref(c2, v2, TOP_DOWN[None], [[0.0, 0.0, 0.08]], 0.005, GRIPPER[4])
    print("one view: counts %s values %s unseen %.3f; two views: counts %s values %s unseen %.3f"
          % (c1[0].tolist(), v1[0].tolist(), d1["grasp_unseen"][0], c2[0].tolist(), v2[0].tolist(), d2["grasp_unseen"][0]))
    S = f32(0.02)
    # one view: no seen surface touches the hand or its sweep, but the far finger stands in unseen space: no safe retreat at all
    assert c1[0, 2] == 0 and c1[0, 4] == 0 and v1[0, 2] == S
    assert c1[0, 3] > 0 and c1[0, 5] > 0 and v1[0, 3] == 0.0 and v1[0, 3] != v1[0, 2]
    assert d1["grasp_unseen"][0] > 0.0 and d1["grasp_clearance_safe"][0] != d1["grasp_clearance_seen"][0]
    blocked = ref.derived_ref(c1, v1, TOP_DOWN[None], [[0.0, 0.0, 0.08]], 0.005, GRIPPER[4], unseen="blocked")
    assert blocked["grasp_clearance"][0] == 0.0 and d1["grasp_clearance"][0] == S
    assert ref.passes_ref(d1, min_clearance=0.02).tolist() == [True] and ref.passes_ref(blocked, min_clearance=0.02).tolist() == [False]
    # two views: the hand and its sweep are seen free, both clearances are the standoff
    assert d2["grasp_unseen"][0] < d1["grasp_unseen"][0] and c2[0, 3] == 0 and c2[0, 5] == 0
    assert v2[0, 2] == S and v2[0, 3] == S and c2[0, 6] == c1[0, 6] and c2[0, 7] == 0


def test_the_closing_width_of_the_fused_box_is_its_true_width_within_a_step_and_a_voxel(fused):
    """The bound.  The grasp is centred on y = 0 with the identity for ``to_volume`` and h = voxel, and the volume's y faces are
    multiples of the voxel from -0.10: a sample's y, (j + 0.5) h - hw, IS the centre of the voxel it falls in, and the box's
    faces at y = -+3 cm are voxel faces.  The voxels on either side of a face have their centres half a voxel, 2.5 mm, from it.
    Two PRECONDITIONS are checked below on the volume itself, in the columns the region reads:
    (1) below the band of the top face, the voxel just inside a side face has D < 0 and the one just outside D >= 0 -- the
        distance error of a view (tests/test_tsdf_reference_cpu.py's E = 0.5 (z / f) tan(slant), under 1.5 mm here at f = 240,
        z = 0.46 m, 52 degrees) is below those 2.5 mm;
    (2) no voxel whose centre is further out than that first outside one is solid in any row: the negative band a slanted view
        leaves behind the top face reaches sideways past the edge (it is ``trunc`` deep along the ray), and the view from the
        other side, which sees those voxels as free, takes back all of it but at most the first voxel.
    With (1) y_max >= 3 cm - voxel / 2 and with (2) y_max <= 3 cm + voxel / 2, likewise y_min: y_max - y_min lies within one
    voxel = one lattice step of the true 6 cm, which is inside the (step + voxel) asked for."""
    vol, (_, two) = fused
    L = ref.rows_of(TOP_DOWN[None], [[0.0, 0.0, 0.08]])
    counts, values = _run(vol, two, L)
    D, Wt = two
    nx, ny, _ = vol.dims
    iy_in, iy_out = int(round((0.0275 + 0.10) / VOXEL - 0.5)), int(round((0.0325 + 0.10) / VOXEL - 0.5))
    ix = [int(round((v + 0.12) / VOXEL - 0.5)) for v in (-0.0025, 0.0025)]                  # |local z| < ht: world x
    for iz in range(int(round((0.02 + 0.015) / VOXEL)), int(round((0.055 + 0.015) / VOXEL))):   # below the top's band
        for i in ix:
            for inside, outside in ((iy_in, iy_out), (ny - 1 - iy_in, ny - 1 - iy_out)):
                a, b = (iz * ny + inside) * nx + i, (iz * ny + outside) * nx + i
                assert Wt[a] >= 1 and Wt[b] >= 1 and D[a] < 0 and D[b] >= 0, (iz, i, inside, D[a], D[b])
    for iz in range(int(round((0.02 + 0.015) / VOXEL)), int(round((0.14 + 0.015) / VOXEL))):    # every row of the region
        for i in ix:
            for j in list(range(0, ny - 1 - iy_out)) + list(range(iy_out + 1, ny)):
                v = (iz * ny + j) * nx + i
                assert not (Wt[v] >= 1 and D[v] < 0), (iz, i, j, D[v])
    width = float(values[0, 1]) - float(values[0, 0])
    print("closing width %.4f m of a %.4f m box (y_min %.4f, y_max %.4f), region solid / unseen %d / %d"
          % (width, 2 * BOX_HALF_Y, values[0, 0], values[0, 1], counts[0, 0], counts[0, 1]))
    assert counts[0, 0] > 0
    assert abs(width - 2 * BOX_HALF_Y) <= VOXEL + VOXEL                                    # one lattice step plus one voxel
    assert 2 * BOX_HALF_Y - VOXEL - 1e-6 <= width <= 2 * BOX_HALF_Y + VOXEL + 1e-6         # and what the derivation says
    derived = ref.derived_ref(counts, values, TOP_DOWN[None], [[0.0, 0.0, 0.08]], 0.005, GRIPPER[4])
    assert abs(derived["grasp_offset"][0]) < 1e-6 and abs(derived["grasp_opening"][0] - (width + 0.01)) < 1e-6


def test_the_clearance_in_front_of_a_rendered_wall_is_the_analytic_distance():
    """A wall in the plane y = 2 cm faces the camera at y = -35 cm.  The hand points AT the camera (approach -y) from a centre at
    y = -6 cm, so its back face is at y = 0 and its retreat runs towards +y, into the seen face: 2 cm of clearance.

    The bound.  The first solid voxel along the retreat has its lower face b within voxel / 2 + E of the wall (its centre is the
    first one behind the zero crossing, which is within E of the wall); the first sample at or behind b is less than a step
    further: clearance - 2 cm lies in [-voxel / 2 - E, voxel / 2 + E + step).  E = 0.5 (z / f) tan(slant) (tests/
    test_tsdf_reference_cpu.py) = 0.5 * (0.47 / 240) * tan(38 deg) = 0.8 mm, below voxel / 2: within a step plus a voxel."""
    scene = [rectangle((-0.5, -0.5, 0.0), (1.0, 0, 0), (0, 1.0, 0)), rectangle((-0.5, 0.02, 0.0), (1.0, 0, 0), (0, 0, 0.5))]
    vol = tsdf_ref.Volume(**SMALL)
    vol.integrate(render(scene, W, H, K, CAMERAS[0]), None, W, H, K, CAMERAS[0])
    frame = np.array([[0.0, 1.0, 0.0], [-1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])    # columns: approach -y, closing +x, minor +z
    L = ref.rows_of(frame[None], [[0.0, -0.06, 0.08]])
    counts, values = _run(vol, (vol.D, vol.W), L, standoff=0.05)
    print("wall: counts %s values %s" % (counts[0].tolist(), values[0].tolist()))
    assert 0.5 * (0.47 / K[0]) * np.tan(np.radians(38.0)) < VOXEL / 2
    assert counts[0, 4] > 0 and abs(float(values[0, 2]) - 0.02) <= VOXEL + VOXEL
    assert values[0, 3] <= values[0, 2]                  # what is unseen can only shorten the retreat
    # twice the step: the answer moves by less than the coarser step and stays within ITS bound
    _, coarse = _run(vol, (vol.D, vol.W), L, standoff=0.05, step=2 * VOXEL)
    assert abs(float(coarse[0, 2]) - 0.02) <= 2 * VOXEL + VOXEL


# ---- one hand-built volume per rule --------------------------------------------------------------------------------------------
# Dyadic numbers throughout, so that every coordinate is exact and the answers can be written down by hand: the box of
# approach_reference.DYADIC_BOX, S = 0.5, h = voxel = 0.25 and a 6 x 8 x 1 volume whose voxel centres ARE the 48 samples
# (x = -0.875 .. 0.375, y = -0.875 .. 0.875, z = 0) under the identity.  By hand: region 24 (|y| < 0.75, -0.5 < x < 0.5), back 16,
# finger 8, blockers 24 (inner, x < 0) + 12 (the lanes, x < 0.5): 60 memberships.
DYADIC_BOX = (-0.5, 0.5, 0.125, 1.0, 0.75, 0.0)
IDENTITY_L = np.eye(4, dtype=np.float32)[:3].reshape(1, 12)


def _dyadic(min_weight=1):
    return ref.HandVolume((6, 8, 1), (-1.0, -1.0, -0.125), 0.25, trunc=1.0, min_weight=min_weight)


def _ix(x):
    return int((x + 1.0) / 0.25)


def _iy(y):
    return int((y + 1.0) / 0.25)


def _dy(vol, margin=0.0, L=IDENTITY_L, box=DYADIC_BOX, standoff=0.5):
    counts, values = vol.run(L, box, standoff, 0.25, box[1] if not np.ndim(box[1]) else 0.5, margin)
    return counts[0].tolist(), values[0].tolist()


def test_lattice_counts_and_samples():
    assert ref.lattice_counts(DYADIC_BOX, 0.5, 0.25, 0.5)[0] == (6, 8, 1)
    xv, yv, zv = ref.lattice_samples(DYADIC_BOX, 0.5, 0.25, 0.5)
    assert xv.tolist() == [-0.875, -0.625, -0.375, -0.125, 0.125, 0.375] and zv.tolist() == [0.0] and yv[0] == -0.875 and yv[-1] == 0.875
    assert ref.lattice_counts(DYADIC_BOX, 0.5, 8.0, 0.5)[0] == (1, 1, 1)            # a step larger than the box: one sample per axis
    assert ref.lattice_counts(DYADIC_BOX, 0.0, 0.25, -2.0)[0][0] == 1               # an extent that is not positive: one
    # the reference's gripper at a 2 mm step, and at 5 mm, where the float32 constants decide: 0.05f + 0.05f over 0.005f is above 20
    assert ref.lattice_counts(GRIPPER, 0.10, 0.002, 0.06)[0] == (110, 50, 5)
    assert ref.lattice_counts(GRIPPER, 0.02, 0.005, 0.06)[0] == (28, 21, 2)


def test_every_voxel_seen_free_and_nothing_observed():
    free = _dyadic().observe_all(1.0)
    assert _dy(free) == ([0, 0, 0, 0, 0, 0, 60, 0], [inf, -inf, 0.5, 0.5])          # D == 1 is FREE
    assert _dy(_dyadic().observe_all(0.0)) == ([0, 0, 0, 0, 0, 0, 60, 0], [inf, -inf, 0.5, 0.5])   # D == d_solid == 0: strict
    unknown = _dyadic()                                                               # W = 0 everywhere
    assert _dy(unknown) == ([0, 24, 0, 24, 0, 36, 60, 0], [inf, -inf, 0.5, 0.0])
    solid = _dyadic().observe_all(-0.5)
    assert _dy(solid) == ([24, 0, 24, 0, 36, 0, 60, 0], [-0.625, 0.625, 0.0, 0.0])


def test_solid_rule_at_the_threshold_with_and_without_a_margin():
    voxel = (_ix(-0.875), _iy(0.125), 0)                                             # an inner blocker 0.375 behind the palm's back
    for margin, d_solid in ((0.0, f32(0.0)), (0.25, f32(0.25))):                     # trunc = 1: d_solid = margin
        seen = []
        for d in (np.nextafter(d_solid, f32(-np.inf)), d_solid, np.nextafter(d_solid, f32(np.inf))):
            vol = _dyadic().observe_all(1.0)
            vol.D[vol.at(*voxel)] = d
            counts, values = _dy(vol, margin=margin)
            seen.append((counts[4], values[2], values[3]))
        assert seen == [(1, 0.375, 0.375), (0, 0.5, 0.5), (0, 0.5, 0.5)], (margin, seen)
    # -0.0 is not below 0
    vol = _dyadic().observe_all(1.0)
    vol.D[vol.at(*voxel)] = f32(-0.0)
    assert _dy(vol)[0][4] == 0


@pytest.mark.parametrize("min_weight", [1, 2, 3])
def test_unknown_rule_at_min_weight_and_a_nan_distance(min_weight):
    voxel = (_ix(-0.625), _iy(-0.375), 0)                                            # an inner blocker 0.125 behind the back
    for w, expected in ((min_weight - 1, ([0, 0, 0, 0, 0, 1, 60, 0], [inf, -inf, 0.5, 0.125])),
                        (min_weight, ([0, 0, 0, 0, 1, 0, 60, 0], [inf, -inf, 0.125, 0.125]))):
        vol = _dyadic(min_weight).observe_all(1.0, w=min_weight)
        vol.D[vol.at(*voxel)], vol.W[vol.at(*voxel)] = f32(-1.0), w
        assert _dy(vol) == expected, w
    vol = _dyadic(min_weight).observe_all(1.0, w=min_weight)
    vol.D[vol.at(*voxel)] = f32(np.nan)                                              # observed, but no distance: UNKNOWN
    assert _dy(vol) == ([0, 0, 0, 0, 0, 1, 60, 0], [inf, -inf, 0.5, 0.125])


def test_region_hand_and_lane_voxels():
    vol = _dyadic().observe_all(1.0)
    vol.D[vol.at(_ix(0.125), _iy(0.375), 0)] = f32(-0.5)            # between the fingers: region only
    vol.D[vol.at(_ix(0.375), _iy(-0.625), 0)] = f32(-0.5)
    assert _dy(vol) == ([2, 0, 0, 0, 0, 0, 60, 0], [-0.625, 0.375, 0.5, 0.5])
    vol.D[vol.at(_ix(-0.125), _iy(0.125), 0)] = f32(-0.5)           # inside the palm: region, back and a blocker with s = 0
    assert _dy(vol) == ([3, 0, 1, 0, 1, 0, 60, 0], [-0.625, 0.375, 0.0, 0.0])
    vol = _dyadic().observe_all(1.0)
    vol.D[vol.at(_ix(0.375), _iy(0.875), 0)] = f32(-0.5)            # inside a finger: finger and a lane blocker
    assert _dy(vol) == ([0, 0, 1, 0, 1, 0, 60, 0], [inf, -inf, 0.0, 0.0])
    vol.D[vol.at(_ix(-0.375), _iy(-0.875), 0)] = f32(-0.5)          # the lane beside the palm: back AND finger: two memberships
    assert _dy(vol)[0] == [0, 0, 3, 0, 2, 0, 60, 0]


def test_outside_samples_a_shifted_volume_and_a_row_of_nans():
    free = _dyadic().observe_all(1.0)
    shift = IDENTITY_L.copy()
    shift[0, 3] = 0.25                                               # every sample one voxel along +x: the last column leaves
    counts, values = _dy(free, L=shift)
    # x = 0.375 leaves: of its 8 samples 6 are region only, the 2 lane ones are finger + blocker: 4 memberships
    assert counts == [0, 6, 0, 2, 0, 2, 60, 4] and values == [inf, -inf, 0.5, 0.0]
    far = IDENTITY_L.copy()
    far[0, 7] = 100.0                                                # a volume wholly outside the hand
    assert _dy(free, L=far) == ([0, 24, 0, 24, 0, 36, 60, 60], [inf, -inf, 0.5, 0.0])
    for bad in (np.nan, np.inf, -np.inf):
        row = IDENTITY_L.copy()
        row[0, 5] = bad
        assert _dy(free, L=row) == ([0, 24, 0, 24, 0, 36, 60, 60], [inf, -inf, 0.5, 0.0])
    # samples exactly on the volume's faces, by a shift along x (the volume spans [-1, 0.5), voxel 0.25, n = 6).  The memberships
    # of the lowest column of samples are its 8 blockers, those of the highest its 2 lane samples' finger + blocker
    for dx, outside in ((-0.125, 0),                                 # -0.875 -> -1.0, ON the low face: index 0, inside
                        (-0.375, 8),                                 # -0.875 -> -1.25: index -1; -0.625 -> -1.0: index 0
                        (0.0625, 0),                                 # 0.375 -> 0.4375: index n - 1
                        (0.125, 4)):                                 # 0.375 -> 0.5, ON the high face: index n, outside
        row = IDENTITY_L.copy()
        row[0, 3] = dx
        assert _dy(free, L=row)[0][7] == outside, dx


def test_per_grasp_depth_and_no_standoff():
    solid = _dyadic().observe_all(-0.5)
    box = (-0.5, np.array([0.5, 0.125], dtype=np.float32), 0.125, 1.0, 0.75, 0.0)
    counts, values = solid.run(np.repeat(IDENTITY_L, 2, axis=0), box, 0.5, 0.25, 0.5)
    assert counts[0].tolist() == [24, 0, 24, 0, 36, 0, 60, 0]
    # xh = 0.125: close is x in {-0.375, -0.125}: region 12, back 16, finger 4, lane blockers x < 0.125: 4 x 2 -> 24 + 8
    assert counts[1].tolist() == [12, 0, 20, 0, 32, 0, 52, 0] and values[1].tolist() == [-0.625, 0.625, 0.0, 0.0]
    # S = 0: xs = x_lo, n_x = 4; nothing behind the palm's back is a sample
    counts, values = solid.run(IDENTITY_L, DYADIC_BOX, 0.0, 0.25, 0.5)
    assert ref.lattice_counts(DYADIC_BOX, 0.0, 0.25, 0.5)[0] == (4, 8, 1)
    assert counts[0].tolist() == [24, 0, 24, 0, 12 + 8, 0, 44, 0] and values[0].tolist() == [-0.625, 0.625, 0.0, 0.0]
    free = _dyadic().observe_all(1.0)
    _, values = free.run(IDENTITY_L, DYADIC_BOX, 0.0, 0.25, 0.5)
    assert values[0].tolist() == [inf, -inf, 0.0, 0.0] and not np.signbit(values[0, 2:]).any()


# ---- the host side ---------------------------------------------------------------------------------------------------------------
def test_params_defaults_and_validation():
    from regnet_for_3d_grasping_amd import approach
    p = approach.ApproachParams()
    assert (p.space, p.unseen, p.step, p.margin) == ("cloud", "free", None, 0.0)
    assert approach.ApproachParams.coerce({"space": "volume", "unseen": "blocked", "step": 0.004, "margin": 0.002}).space == "volume"
    for bad in ({"space": "mesh"}, {"unseen": "maybe"}, {"step": 0.0}, {"step": float("nan")}, {"step": 1e-60}, {"step": float("inf")},
                {"margin": -1e-3}, {"margin": float("nan")}, {"margin": float("inf")}):
        with pytest.raises(ValueError, match="approach: %s" % next(iter(bad))):
            approach.ApproachParams(**bad)


def test_the_product_lattice_equals_the_restatements():
    from regnet_for_3d_grasping_amd import approach_volume, eval_collision
    for depth, standoff, step, extent in ((0.06, 0.10, 0.002, 0.06), (0.06, 0.0, 0.005, 0.09), (0.03, 0.05, 1.0, 0.03)):
        box = eval_collision._box_args(depth, WIDTH, 1, None)[0]
        assert approach_volume.lattice(box, standoff, step, extent) == ref.lattice_counts(ref.gripper_box(depth, WIDTH), standoff, step, extent)[0]
    assert approach_volume.MAX_SAMPLES == ref.MAX_SAMPLES


def test_cli_flags_reach_the_params():
    from regnet_for_3d_grasping_amd import approach, detect
    parser = detect.build_parser()
    required = ["--folder", "f", "--load-score-path", "s", "--load-region-path", "r"]
    assert detect.approach_from_args(parser.parse_args(required)) is None
    args = parser.parse_args(required + ["--approach-space", "volume", "--approach-unseen", "blocked", "--approach-step", "0.004",
                                         "--approach-margin", "0.002", "--tsdf"])
    given = detect.approach_from_args(args)
    assert given == {"space": "volume", "unseen": "blocked", "step": 0.004, "margin": 0.002}
    p = approach.ApproachParams.coerce(given)
    assert (p.space, p.unseen, p.step, p.margin) == ("volume", "blocked", 0.004, 0.002)
    with pytest.raises(SystemExit):
        parser.parse_args(required + ["--approach-space", "mesh"])
    assert detect.APPROACH_VOLUME_KEYS == ("grasp_clearance_seen", "grasp_clearance_safe", "grasp_unseen", "grasp_solid_hand")


def test_the_header_declares_the_entry_point_and_it_refuses_before_any_launch():
    """The argument checks come before any launch, so they run without a GPU."""
    from regnet_for_3d_grasping_amd import _lib
    name = "regnet_grasp_approach_volume_f32"
    assert _lib.PARAMS[name][-1] == "stream" and len(_lib.PARAMS[name]) == 24
    origin = (ctypes.c_float * 3)(0.0, 0.0, 0.0)
    fake = ctypes.c_void_p(16)                                      # never read: every call below returns before a launch

    def raw(volume=fake, dims=(4, 4, 4), origin3=origin, voxel=0.25, trunc=1.0, min_weight=1, margin=0.0, L=fake, B=1, standoff=0.5,
            step=0.25, x_extent=0.5, counts=fake, values=fake, hw=1.0):
        return _lib.lib.regnet_grasp_approach_volume_f32(volume, dims[0], dims[1], dims[2], origin3, voxel, trunc, min_weight, margin, L, B,
                                                         -0.5, 0.5, None, 0.125, hw, 0.75, 0.0, standoff, step, x_extent, counts,
                                                         values, None)

    assert raw(B=-1) == -1 and raw(dims=(0, 4, 4)) == -1 and raw(dims=(4, 4, -1)) == -1 and raw(min_weight=0) == -1
    assert raw(dims=(1 << 10, 1 << 10, 1 << 9)) == -3 and raw(dims=((1 << 24) + 1, 1, 1)) == -3 and raw(B=1 << 31) == -3
    for name_ in ("voxel", "trunc", "step"):
        for bad in (0.0, -1.0, float("nan"), float("inf"), 1e-60, 1e60):
            assert raw(**{name_: bad}) == -3, (name_, bad)
    assert raw(standoff=-1e-3) == -3 and raw(standoff=float("nan")) == -3 and raw(standoff=float("inf")) == -3
    assert raw(margin=float("nan")) == -3 and raw(margin=float("inf")) == -3
    assert raw(step=2.0 ** -12, x_extent=3.0) == -3                  # 16384 x 8192 x 1024 samples: more than 2^22
    assert raw(step=0.25 * 2.0 ** -6, standoff=15.5, hw=16.0) == -3  # 1056 x 2048 x 64 samples: each count small, the product not
    assert raw(x_extent=float("nan")) == -3 and raw(x_extent=float("inf")) == -3 and raw(hw=float("nan")) == -3
    assert raw(B=0, volume=None, L=None) == 0                        # nothing to do comes before the pointers
    for null in ("volume", "origin3", "L", "counts", "values"):
        assert raw(**{null: None}) == -2, null
