"""tests/sdf_reference.py, the all-pairs numpy restatement of the signed, capped distance field, held to things it can be wrong
about: scipy's exact Euclidean transform of the mask and of its complement, planted ties on both sides, its relation to
tests/edt_reference.py, the cap, and what the interpolated query reads next to a wall -- a hand-set wall through a voxel face,
where it must be the true signed distance up to rounding, and a slanted rendered wall, where the bound is derived below.  No GPU.

The volume is tests/tsdf_reference.py's, the view is tests/icp_projective_reference.py's analytic renderer.
"""
import numpy as np
import pytest

from . import edt_reference as edt_ref
from . import sdf_reference as ref
from . import tsdf_reference as tsdf_ref
from .icp_projective_reference import look_at, rectangle, render

f32 = np.float32
NONE = ref.NONE
EPS = 2.0 ** -24
IDENTITY = np.eye(4, dtype=np.float32)[:3].reshape(12)


def _at(dims, ix, iy, iz):
    return (iz * dims[1] + iy) * dims[0] + ix


def _mask(dims, voxels):
    m = np.zeros((dims[0] * dims[1] * dims[2],), dtype=bool)
    for v in voxels:
        m[_at(dims, *v)] = True
    return m


@pytest.mark.parametrize("density", [0.002, 0.05, 0.5, 0.97])
def test_both_sides_equal_scipy_on_random_masks(density):
    ndimage = pytest.importorskip("scipy.ndimage")
    dims = (24, 17, 9)
    rng = np.random.default_rng(int(density * 1000) + 11)
    mask = rng.random(dims[0] * dims[1] * dims[2]) < density
    assert mask.any() and not mask.all()
    field, nearest = ref.transform(mask, dims)
    lattice = mask.reshape(dims[2], dims[1], dims[0])
    positive = np.rint(ndimage.distance_transform_edt(~lattice) ** 2).astype(np.int64).reshape(-1)
    negative = np.rint(ndimage.distance_transform_edt(lattice) ** 2).astype(np.int64).reshape(-1)
    assert np.array_equal(field, np.where(mask, -negative, positive))
    assert (field != 0).all() and (field[mask] <= -1).all() and (field[~mask] >= 1).all()
    # every nearest is a voxel of the OTHER class at exactly |field|
    xyz = edt_ref.coords(dims)
    assert np.array_equal(mask[nearest], ~mask)
    assert np.array_equal(((xyz - xyz[nearest]) ** 2).sum(axis=1), np.abs(field))


def test_planted_ties_on_both_sides_go_to_the_smallest_linear_index():
    dims = (3, 3, 3)
    faces = [(0, 1, 1), (2, 1, 1), (1, 0, 1), (1, 2, 1), (1, 1, 0), (1, 1, 2)]
    centre = _at(dims, 1, 1, 1)
    field, nearest = ref.transform(_mask(dims, faces), dims)          # a free voxel between six obstacles
    assert field[centre] == 1 and nearest[centre] == _at(dims, 1, 1, 0)
    field, nearest = ref.transform(~_mask(dims, faces), dims)         # an obstacle among six free voxels (the rest solid)
    assert field[centre] == -1 and nearest[centre] == _at(dims, 1, 1, 0)
    # 0 + 25 = 9 + 16: (5, 0) and (3, 4) from the origin of a plane, on either side
    dims = (6, 5, 1)
    pair = _mask(dims, [(5, 0, 0), (3, 4, 0)])
    field, nearest = ref.transform(pair, dims)
    assert field[0] == 25 and nearest[0] == _at(dims, 5, 0, 0)
    field, nearest = ref.transform(~pair, dims)
    assert field[0] == -25 and nearest[0] == _at(dims, 5, 0, 0)
    assert field[_at(dims, 5, 0, 0)] == 1 and field[_at(dims, 3, 4, 0)] == 1


def test_no_obstacle_and_no_free_voxel():
    dims = (4, 3, 2)
    field, nearest = ref.transform(np.zeros((24,), dtype=bool), dims)
    assert (field == NONE).all() and (nearest == -1).all()
    field, nearest = ref.transform(np.ones((24,), dtype=bool), dims)
    assert (field == -NONE).all() and (nearest == -1).all()
    field, nearest = ref.transform(np.ones((24,), dtype=bool), dims, cap=3)
    assert (field == -9).all() and (nearest == -1).all()
    field, nearest = ref.transform(np.zeros((24,), dtype=bool), dims, outside=True, cap=1)
    assert (field == 1).all()                         # min(m^2, 1) with m >= 1


@pytest.mark.parametrize("outside", [False, True])
def test_relations_to_the_unsigned_restatement(outside):
    dims = (13, 9, 6)
    mask = np.random.default_rng(5).random(13 * 9 * 6) < 0.04
    want = edt_ref.transform(mask, dims, outside)
    got = ref.transform(mask, dims, outside, sign=0, cap=0)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    signed = ref.transform(mask, dims, outside, sign=1, cap=0)
    assert np.array_equal(signed[0][~mask], want[0][~mask]) and np.array_equal(signed[1][~mask], want[1][~mask])
    assert (signed[0][mask] < 0).all()
    # the outside is never free space: the negative side does not see it
    inner = edt_ref.transform(~mask, dims, False)
    assert np.array_equal(signed[0][mask], -inner[0][mask]) and np.array_equal(signed[1][mask], inner[1][mask])


def test_the_cap_saturates_and_a_distance_of_exactly_the_cap_keeps_its_nearest():
    dims = (12, 9, 1)
    mask = _mask(dims, [(0, 0, 0)])
    free, near = ref.transform(mask, dims, cap=5)
    assert free[_at(dims, 5, 0, 0)] == 25 and near[_at(dims, 5, 0, 0)] == 0          # exactly the cap along one axis
    assert free[_at(dims, 3, 4, 0)] == 25 and near[_at(dims, 3, 4, 0)] == 0          # exactly the cap, 9 + 16
    assert free[_at(dims, 4, 4, 0)] == 25 and near[_at(dims, 4, 4, 0)] == -1         # 32 saturates, strictly beyond
    assert free[_at(dims, 6, 0, 0)] == 25 and near[_at(dims, 6, 0, 0)] == -1
    uncapped, _ = ref.transform(mask, dims)
    assert np.array_equal(free, np.clip(uncapped, -25, 25))


def test_signed_metres_are_linear_across_a_wall():
    words = np.array([-9, -4, -1, 1, 4, 9, NONE, -NONE], dtype=np.int32)
    got = ref.metres_signed_ref(words, 0.25)
    assert got.dtype == np.float32
    assert got.tolist() == [-0.625, -0.375, -0.125, 0.125, 0.375, 0.625, np.inf, -np.inf]


# ---- a hand-set wall through a voxel face -------------------------------------------------------------------------------------
WALL_DIMS = (12, 6, 5)
WALL_K = 7                                  # the obstacles are the voxels with ix >= 7: the face is the plane x = origin + 7 voxel


@pytest.mark.parametrize("voxel,origin", [(0.25, (-1.0, -1.0, -0.5)), (0.005, (-0.031, 0.017, 0.4))])
def test_the_interpolated_distance_across_a_wall_through_a_voxel_face_is_the_true_one(voxel, origin):
    """Rounding bound.  Every corner value is (k - 0.5) voxel_f, k an integer: the root and the subtraction are exact, the
    product is rounded once.  u = (w - o) / voxel_f - 0.5 takes three roundings of numbers below n = 12, so t is off by at most
    3 eps n, which moves a lerp along x by 3 eps n voxel (|b - a| = voxel); the lerps along y and z join equal values.  Each of
    the nine roundings of the three lerps is at most eps times the largest magnitude, n voxel.  With the rounding of voxel
    itself (eps n voxel) and of the product (eps n voxel) that is 14 eps n voxel; the bound held is 16 eps n voxel, and for the
    gradient, whose exact value is the wall's normal (-1, 0, 0) and which goes through one division more, 16 eps n."""
    dims = WALL_DIMS
    ix = edt_ref.coords(dims)[:, 0]
    mask = ix >= WALL_K
    field, _ = ref.transform(mask, dims)
    o = np.asarray(origin, dtype=np.float32)
    vx = float(f32(voxel))
    rng = np.random.default_rng(3)
    lo = o.astype(np.float64) + vx                       # at least one voxel from the rim
    hi = o.astype(np.float64) + (np.array(dims) - 1.0) * vx
    points = (lo + rng.random((400, 3)) * (hi - lo)).astype(np.float32)
    distance, gradient, _ = ref.query_signed_ref(field, None, dims, o, voxel, points, IDENTITY, interpolate=True)
    true = (float(o[0]) + WALL_K * vx) - points[:, 0].astype(np.float64)
    tol = 16 * EPS * dims[0] * vx
    print("face wall: max |distance - true| = %.3g, bound %.3g" % (np.abs(distance - true).max(), tol))
    assert (true < 0).any() and (true > 0).any()
    assert np.all(np.abs(distance - true) <= tol)
    assert np.all(np.abs(gradient - np.array([-1.0, 0.0, 0.0])) <= 16 * EPS * dims[0])
    # at a voxel centre the corner value comes back exactly
    centres = (o[None, :] + (edt_ref.coords(dims).astype(np.float32) + f32(0.5)) * f32(voxel)).astype(np.float32)
    at, _, _ = ref.query_signed_ref(field, None, dims, o, voxel, centres, IDENTITY, interpolate=False)
    assert np.array_equal(at, ref.metres_signed_ref(field, voxel))


# ---- a slanted rendered wall --------------------------------------------------------------------------------------------------
W, H = 256, 192
K = (240.0, 240.0, 127.5, 95.5)
VOXEL = 0.005
TRUNC = 0.02
SMALL = dict(voxel=VOXEL, trunc=TRUNC, origin=(-0.12, -0.10, -0.015), dims=(48, 40, 36), max_points=1 << 14)
CAMERA = look_at((0.0, -0.35, 0.30), (0.0, 0.0, 0.03))
WALL_Y = 0.02
SLOPE = np.radians(20.0)                    # the wall is turned about z by this: its normal is (sin, -cos, 0), towards the camera
INCIDENCE = np.radians(50.0)                # no ray meets the slanted wall at more than this from its normal in this view
E = 0.5 * (0.47 / K[0]) * np.tan(INCIDENCE)  # the volume's surface error at that incidence (tests/test_tsdf_reference_cpu.py's rule)
# The bound, with t(x) the true signed distance of x to the wall (positive in front) and v the voxel.
#  (a) A voxel is solid only if its centre q lies behind the depth the view measured, which is within E of the wall: t(q) <= E.
#      So a free voxel's centre c has |c - q| >= t(c) - E for every obstacle q: its value is >= t(c) - E - v / 2.
#  (b) A centre q with -TRUNC cos(INCIDENCE) + E <= t(q) <= -E is observed (within the truncation along the ray) and behind the
#      wall: solid.  The wall runs along z, so within c's own z layer the centres form a square lattice, whose covering radius is
#      v / sqrt 2: the point E + v / sqrt 2 behind the foot of c's perpendicular has a centre q within v / sqrt 2, whose t(q) lies
#      in [-E - sqrt 2 v, -E], inside the band as long as TRUNC cos(INCIDENCE) >= 2 E + sqrt 2 v (asserted).  It is at most
#      t(c) + E + sqrt 2 v from c: the value of c is <= t(c) + E + (sqrt 2 - 1 / 2) v.
#  (c) t is linear, so where all eight corners are free voxels the trilinear interpolant of t at the corners is t at the point,
#      and the interpolant of the values is off by a convex combination of the corners' errors:
#          -(E + v / 2) <= distance - t <= E + (sqrt 2 - 1 / 2) v,   |distance - t| <= E + 0.915 v   (+ 1e-6 for float32)
#  The slope enters through E (the incidence) and through the lattice argument, which holds for any turn about z; at slope 0 the
#  first solid centre of c's own row is within v of the crossing and the bound falls to E + v / 2.  The unsigned nearest-voxel
#  lookup on the same points is held to 1.5 v + E (tests/test_edt_reference_cpu.py): this bound is tighter by 0.585 v.
SLANT_BOUND = E + (np.sqrt(2.0) - 0.5) * VOXEL + 1e-6
UNSIGNED_BOUND = 1.5 * VOXEL + E


@pytest.fixture(scope="module")
def slanted():
    u = np.array([np.cos(SLOPE), np.sin(SLOPE), 0.0])
    corner = np.array([0.0, WALL_Y, 0.0]) - 0.5 * u
    scene = [rectangle((-0.5, -0.5, 0.0), (1.0, 0, 0), (0, 1.0, 0)), rectangle(tuple(corner), tuple(u), (0, 0, 0.5))]
    vol = tsdf_ref.Volume(**SMALL)
    vol.integrate(render(scene, W, H, K, CAMERA), None, W, H, K, CAMERA)
    mask = edt_ref.obstacle_mask(vol.D, vol.W, vol.p["trunc"], vol.p["min_weight"], 0.0, 0)
    assert mask.sum() > 1000
    return vol, mask


def test_the_interpolated_distance_in_front_of_a_slanted_rendered_wall(slanted):
    vol, mask = slanted
    assert TRUNC * np.cos(INCIDENCE) >= 2 * E + np.sqrt(2.0) * VOXEL
    assert SLANT_BOUND < UNSIGNED_BOUND
    normal = np.array([np.sin(SLOPE), -np.cos(SLOPE), 0.0])
    along = np.array([np.cos(SLOPE), np.sin(SLOPE), 0.0])
    foot = np.array([0.0, WALL_Y, 0.0])
    points = np.array([foot + s * along + gap * normal + np.array([0.0, 0.0, z])
                       for gap in (0.0112, 0.0163, 0.02, 0.0271, 0.034) for s in (-0.03, -0.0031, 0.012)
                       for z in (0.07, 0.0833)], dtype=np.float32)       # at least 7 cm above the table: the wall is nearer
    inside, v = edt_ref.lookup(points, IDENTITY, vol.dims, vol.origin, VOXEL)
    assert inside.all()
    nx, ny, _ = vol.dims
    around = (v[:, None] + np.array([(dz * ny + dy) * nx + dx for dz in (-1, 0, 1) for dy in (-1, 0, 1) for dx in (-1, 0, 1)])[None, :])
    field, nearest = ref.transform(mask, vol.dims, cap=10, at=around.reshape(-1))   # (5 cm: beyond every distance read here)
    distance, _, _ = ref.query_signed_ref(field, nearest, vol.dims, vol.origin, VOXEL, points, IDENTITY, interpolate=True)
    true = (points.astype(np.float64) - foot) @ normal
    # all eight corners are free voxels: the points are at least 2.2 voxels in front of the wall
    assert np.all(true >= 2.2 * VOXEL) and np.all(np.isfinite(distance))
    error = distance - true
    print("slanted wall: distance - true [mm]", np.round(error * 1e3, 2).tolist(), "bound", round(SLANT_BOUND * 1e3, 2),
          "unsigned bound", round(UNSIGNED_BOUND * 1e3, 2))
    assert np.all(error >= -(E + VOXEL / 2 + 1e-6)) and np.all(error <= SLANT_BOUND)
    # the nearest-voxel lookup of the unsigned field on the same points, for comparison: held to its own, wider bound
    coarse, _ = edt_ref.query_ref(np.where(field > 0, field, 0), None, vol.dims, vol.origin, VOXEL, points)
    print("  unsigned nearest-voxel: distance - true [mm]", np.round((coarse - true) * 1e3, 2).tolist())
    assert np.all(np.abs(coarse - true) <= UNSIGNED_BOUND)
