"""tests/edt_reference.py, the all-pairs numpy restatement of the distance field, held to things it can be wrong about: scipy's
exact Euclidean transform on random masks, the tie rule on planted ties, the outside rule, and on a rendered wall the distance
a planner would read -- at a point and as a hand's margin -- against the analytic one.  No GPU.

The volume is tests/tsdf_reference.py's, the view is tests/icp_projective_reference.py's analytic renderer.
"""
import numpy as np
import pytest

from . import approach_volume_reference as av_ref
from . import edt_reference as ref
from . import tsdf_reference as tsdf_ref
from .icp_projective_reference import look_at, rectangle, render

f32 = np.float32
NONE = ref.NONE


def _at(dims, ix, iy, iz):
    return (iz * dims[1] + iy) * dims[0] + ix


def _mask(dims, voxels):
    m = np.zeros((dims[0] * dims[1] * dims[2],), dtype=bool)
    for v in voxels:
        m[_at(dims, *v)] = True
    return m


@pytest.mark.parametrize("density", [0.002, 0.05, 0.5])
def test_all_pairs_equals_scipy_on_random_masks(density):
    ndimage = pytest.importorskip("scipy.ndimage")
    dims = (24, 17, 9)
    rng = np.random.default_rng(int(density * 1000) + 7)
    mask = rng.random(dims[0] * dims[1] * dims[2]) < density
    assert mask.any()
    dist2, nearest = ref.transform(mask, dims)
    lattice = mask.reshape(dims[2], dims[1], dims[0])
    expect = np.rint(ndimage.distance_transform_edt(~lattice) ** 2).astype(np.int64).reshape(-1)
    assert np.array_equal(dist2, expect)
    # every nearest is an obstacle at exactly dist2
    xyz = ref.coords(dims)
    assert mask[nearest].all()
    assert np.array_equal(((xyz - xyz[nearest]) ** 2).sum(axis=1), dist2)


def test_the_six_neighbour_tie_goes_to_the_smallest_linear_index():
    dims = (3, 3, 3)
    faces = [(0, 1, 1), (2, 1, 1), (1, 0, 1), (1, 2, 1), (1, 1, 0), (1, 1, 2)]
    dist2, nearest = ref.transform(_mask(dims, faces), dims)
    centre = _at(dims, 1, 1, 1)
    assert dist2[centre] == 1 and nearest[centre] == _at(dims, 1, 1, 0)


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_a_two_way_tie_along_one_axis_goes_to_the_smaller_coordinate(axis):
    dims = [1, 1, 1]
    dims[axis] = 7
    lo, hi, mid = [0, 0, 0], [0, 0, 0], [0, 0, 0]
    lo[axis], hi[axis], mid[axis] = 1, 5, 3
    dist2, nearest = ref.transform(_mask(dims, [lo, hi]), dims)
    assert dist2[_at(dims, *mid)] == 4 and nearest[_at(dims, *mid)] == _at(dims, *lo)


def test_the_outside_rule_on_an_empty_volume():
    dims = (5, 4, 3)
    dist2, nearest = ref.transform(np.zeros((60,), dtype=bool), dims, outside=True)
    xyz = ref.coords(dims)
    m = np.minimum(xyz + 1, np.array(dims)[None] - xyz).min(axis=1)
    assert np.array_equal(dist2, m * m) and (nearest == -1).all()
    assert dist2[_at(dims, 2, 1, 1)] == 4 and dist2[_at(dims, 0, 0, 0)] == 1
    none, nobody = ref.transform(np.zeros((60,), dtype=bool), dims, outside=False)
    assert (none == NONE).all() and (nobody == -1).all()


def test_a_face_tie_goes_to_the_interior_obstacle():
    dims = (5, 5, 5)
    obstacle = (2, 2, 3)                    # voxel (2, 2, 1): 2 from the obstacle, 2 from the face z = -1
    dist2, nearest = ref.transform(_mask(dims, [obstacle]), dims, outside=True)
    v = _at(dims, 2, 2, 1)
    assert dist2[v] == 4 and nearest[v] == _at(dims, *obstacle)
    w = _at(dims, 2, 2, 0)                  # 1 from the face, 3 from the obstacle: the outside is strictly nearer
    assert dist2[w] == 1 and nearest[w] == -1


def test_classification_follows_the_approach_analysis():
    D = np.array([-0.5, 0.5, np.nan, -0.5, 0.25], dtype=np.float32)
    Wt = np.array([1, 1, 1, 0, 2], dtype=np.int32)
    assert ref.obstacle_mask(D, Wt, 1.0, 1, 0.0, 0).tolist() == [True, False, False, False, False]
    assert ref.obstacle_mask(D, Wt, 1.0, 1, 0.0, 1).tolist() == [True, False, True, True, False]
    assert ref.obstacle_mask(D, Wt, 1.0, 2, 0.5, 0).tolist() == [False, False, False, False, True]


# ---- a rendered wall ------------------------------------------------------------------------------------------------------------
W, H = 256, 192
K = (240.0, 240.0, 127.5, 95.5)
VOXEL = 0.005
SMALL = dict(voxel=VOXEL, trunc=0.01, origin=(-0.12, -0.10, -0.015), dims=(48, 40, 36), max_points=1 << 14)
CAMERA = look_at((0.0, -0.35, 0.30), (0.0, 0.0, 0.03))
WALL_Y = 0.02
E = 0.5 * (0.47 / K[0]) * np.tan(np.radians(38.0))     # the volume's own surface error (tests/test_tsdf_reference_cpu.py)
# The bound.  Every solid voxel's centre lies behind the zero crossing, which is within E of the wall: its y is above WALL_Y - E.
# The first solid voxel of the point's own (x, z) column has its centre at most a voxel behind the crossing: its y is at most
# WALL_Y + E + voxel.  The point's voxel centre is within voxel / 2 of the point along y.  So with t the point's true distance
# to the wall, distance - t lies in [-(voxel / 2 + E), voxel / 2 + voxel + E]: |distance - t| <= 1.5 voxel + E.
POINT_BOUND = 1.5 * VOXEL + E


@pytest.fixture(scope="module")
def wall():
    scene = [rectangle((-0.5, -0.5, 0.0), (1.0, 0, 0), (0, 1.0, 0)), rectangle((-0.5, WALL_Y, 0.0), (1.0, 0, 0), (0, 0, 0.5))]
    vol = tsdf_ref.Volume(**SMALL)
    vol.integrate(render(scene, W, H, K, CAMERA), None, W, H, K, CAMERA)
    mask = ref.obstacle_mask(vol.D, vol.W, vol.p["trunc"], vol.p["min_weight"], 0.0, 0)
    assert mask.sum() > 1000
    return vol, mask


def test_the_distance_in_front_of_a_rendered_wall_is_the_analytic_one(wall):
    vol, mask = wall
    assert E < VOXEL / 2
    points = np.array([[x, WALL_Y - gap, z] for gap in (0.006, 0.013, 0.02, 0.031, 0.04) for x in (-0.03, 0.012)
                       for z in (0.07, 0.083)], dtype=np.float32)        # at least 7 cm above the table: the wall is nearer
    inside, v = ref.lookup(points, np.eye(4, dtype=np.float32)[:3].reshape(12), vol.dims, vol.origin, VOXEL)
    assert inside.all()
    dist2, nearest = ref.transform(mask, vol.dims, at=v)
    distance, xyz = ref.query_ref(dist2, nearest, vol.dims, vol.origin, VOXEL, points)
    true = WALL_Y - points[:, 1].astype(np.float64)
    print("wall: distance - true [mm]", np.round((distance - true) * 1e3, 2).tolist(), "bound", round(POINT_BOUND * 1e3, 2))
    assert np.all(np.abs(distance - true) <= POINT_BOUND)
    assert np.all(xyz[:, 1] > WALL_Y - E) and np.all(xyz[:, 1] <= WALL_Y + E + VOXEL + 1e-6)


def test_a_hand_parallel_to_the_wall_has_the_gap_for_its_margin(wall):
    """The hand hangs top-down with its thin axis along the wall's normal: its face towards the wall is at y = centre + ht, `gap`
    in front of the wall.  The hand's samples are cell centres of step h: the layer nearest the wall is h / 2 inside that face,
    so margin_hand is the point bound away from gap + h / 2: |margin_hand - gap| <= h / 2 + 1.5 voxel + E."""
    vol, mask = wall
    gap, h, standoff = 0.02, VOXEL, 0.01
    box = av_ref.gripper_box(0.06, 0.08)             # x_lo -0.06, x_hi 0.06, ht 0.005, hw 0.05, hs 0.04, back_x -0.0
    ht = float(box[2])
    frame = np.array([[0.0, -1.0, 0.0], [0.0, 0.0, 1.0], [-1.0, 0.0, 0.0]])   # columns: approach -z, closing -x, minor +y
    assert np.allclose(np.cross(frame[:, 0], frame[:, 1]), frame[:, 2])
    L = av_ref.rows_of(frame[None], [[0.0, WALL_Y - gap - ht, 0.10]])
    xv, yv, zv = av_ref.lattice_samples(box, standoff, h, 0.06)
    x, y, z = (a.reshape(-1) for a in np.meshgrid(xv, yv, zv, indexing="ij"))
    inside, v = ref.lookup(np.stack([x, y, z], axis=1), L[0], vol.dims, vol.origin, VOXEL)
    dist2, _ = ref.transform(mask, vol.dims, at=v[inside])
    margins, counts = ref.margin_ref(dist2, vol.dims, vol.origin, VOXEL, 0, L, box, standoff, h, 0.06)
    hand, sweep = ref.metres_ref(margins[0], VOXEL)
    print("hand at %.0f mm: margin_hand %.2f mm, margin_sweep %.2f mm, counts %s" % (gap * 1e3, hand * 1e3, sweep * 1e3,
                                                                                      counts[0].tolist()))
    assert counts[0, 0] > 0 and counts[0, 1] == 0 and counts[0, 2] > counts[0, 0]
    assert abs(float(hand) - gap) <= h / 2 + POINT_BOUND
    assert sweep <= hand
