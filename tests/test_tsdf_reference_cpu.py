"""tests/tsdf_reference.py, the numpy restatement of the TSDF volume's contract, held to things it can be wrong about: where the
surface of a rendered plane and sphere comes out, what five noisy views average to, what free-space evidence removes, and the
hand-built cases of the contract (saturation, the D < 1 rule, the key order, overflow).  No GPU.

eps = 2^-24 is float32's unit roundoff throughout.
"""
import numpy as np
import pytest

from regnet_for_3d_grasping_amd import tsdf          # (host side only: the parameters the restatement's defaults are held to)

from . import tsdf_reference as ref
from .icp_projective_reference import look_at, rectangle, render, sphere

f32 = np.float32
EPS = 2.0 ** -24
W, H = 64, 48
K = (400.0, 400.0, 31.5, 23.5)           # a pixel is 1 mm wide at 0.4 m: half the 2 mm voxel
SMALL = dict(voxel=0.002, trunc=0.01, origin=(-0.02, -0.02, 0.38), dims=(20, 20, 20), max_points=4096)


def constant_depth(z, speckle=None):
    """The organised cloud of a camera that sees the depth ``z`` at every pixel (x, y are not read by the volume)."""
    xyz = np.zeros((H * W, 3), dtype=np.float32)
    xyz[:, 2] = f32(z)
    if speckle is not None:
        xyz[speckle[0], 2] = f32(speckle[1])
    return xyz


def test_fronto_parallel_plane_is_exact_up_to_rounding():
    """A rendered plane at z0 = 0.4137 m (no multiple of the voxel), camera at the common frame's origin.  The depth image is
    constant, so sdf is linear in z and the interpolation exact up to rounding: with |z| <= 0.5 m, a voxel centre carries 2 eps
    |z| (a product and a sum), so the spacing of two centres is off voxel_f by at most 4 eps |z|; zd - pz is exact (Sterbenz); s
    has four roundings (two products by rtrunc, the difference, the division) and s * voxel a fifth: 5 eps voxel; the last sum eps
    |z|; the rendered depth eps |z|.  In all below 10 eps 0.5 m = 3e-7 m.  Along x and y D is constant, so the gradient is (0, 0,
    g) with g < 0 and g / sqrt(g g) = -1 exactly: the normal is held to 4 eps."""
    z0 = 0.4137
    scene = [rectangle((-1.0, -1.0, z0), (2.0, 0, 0), (0, 2.0, 0))]
    xyz = render(scene, W, H, K)
    assert np.isfinite(xyz).all()
    vol = ref.Volume(**SMALL)
    counts = vol.integrate(xyz, None, W, H, K)
    assert counts.sum() == vol.n and counts[ref.UPDATED] > 0
    out = vol.extract()
    k = int(out["num"][0])
    assert k == 400 and out["num"][3] == 0                    # every one of the 20 x 20 columns crosses once
    assert (out["keys"] % 3 == 2).all()                       # z-edges only
    err = np.abs(out["xyz"][:k, 2].astype(np.float64) - z0).max()
    print("plane: max |z - z0| = %.3g m (bound 3e-7)" % err)
    assert err <= 10 * EPS * 0.5
    assert np.abs(out["normal"][:k] - np.array([0, 0, -1], dtype=np.float32)).max() <= 4 * EPS
    assert (out["weight"][:k] == 1).all() and np.isnan(out["xyz"][k:]).all() and (out["weight"][k:] == -1).all()


def _surface_errors(out, poses, distance, normal_of, max_slant_deg):
    """Per extracted row the distance to the true surface and the angle to its normal, and the per-row bounds.

    The bound.  A voxel reads the depth of the NEAREST pixel, up to half a pixel from its own projection in u and in v: at depth
    z that is 0.5 z / f metres sideways each, and on a surface with normal n (in the camera's frame) the depth changes by |n_x| /
    |n_z| and |n_y| / |n_z| per metre: E = 0.5 (z / f) (|n_x| + |n_y|) / |n_z| is the error of one view's sdf.  The mean of two
    views' errors is at most the larger E.  The sdf of a point at distance d from the surface is d cos(b) / cos(a) (b: ray to
    optical axis, a: ray to normal), at least d cos(b) in magnitude, so the zero crossing lies within E / cos(b) of the surface;
    cos(b) >= 0.995 for this 64 x 48 image at f = 400.  A gradient component is a difference of two D values, each off by E, over
    two voxels, against a true gradient of at least cos(b) per metre: the normal is within asin(sqrt(3) E / (voxel cos(b))).  Rows
    that a view sees at more than ``max_slant_deg`` between ray and normal are not held (E grows without bound at a silhouette)."""
    k = int(out["num"][0])
    p = out["xyz"][:k].astype(np.float64)
    n_true = normal_of(p)
    dist = np.abs(distance(p))
    E = np.zeros((k,))
    held = np.ones((k,), dtype=bool)
    for pose in poses:
        R, t = pose[:3, :3], pose[:3, 3]
        n_cam = n_true @ R                                   # R^T n
        z = ((p - t) @ R)[:, 2]
        ray = (p - t) / np.linalg.norm(p - t, axis=1)[:, None]
        slant = np.degrees(np.arccos(np.clip(np.abs((ray * n_true).sum(axis=1)), 0, 1)))
        held &= slant <= max_slant_deg
        with np.errstate(divide="ignore", invalid="ignore"):
            E = np.maximum(E, 0.5 * (z / K[0]) * (np.abs(n_cam[:, 0]) + np.abs(n_cam[:, 1])) / np.abs(n_cam[:, 2]))
    cosb = 0.995
    normal = out["normal"][:k].astype(np.float64)
    angle = np.degrees(np.arccos(np.clip((normal * n_true).sum(axis=1), -1, 1)))
    bound_d = E / cosb + 1e-6
    bound_a = np.degrees(np.arcsin(np.clip(np.sqrt(3.0) * E / (0.002 * cosb), 0, 1))) + 0.1
    return dist, angle, bound_d, bound_a, held


def _two_views(scene, centre):
    poses = [look_at((0.0, 0.0, 0.0), centre, up=(0.0, -1.0, 0.0)), look_at((0.25, 0.0, 0.08), centre, up=(0.0, -1.0, 0.0))]
    clouds = [(render(scene, W, H, K, pose), None) for pose in poses]
    _, counts, out = ref.fuse_volume(clouds, [(W, H, K)] * 2, poses, **SMALL)
    assert out["num"][3] == 0 and out["num"][0] > 100
    return poses, counts, out


def test_slanted_plane_from_two_views():
    """Measured on the restatement: distance at most 0.135 mm against bounds of 0.283 - 0.299 mm, angle at most 4.7 deg against
    14.2 - 15.1 deg (see ``_surface_errors`` for the bound)."""
    n = np.array([0.5, 0.0, -np.sqrt(0.75)])                 # 30 deg to the first camera's axis
    c = np.array([0.0, 0.0, 0.4])
    a = np.cross(n, [0.0, 1.0, 0.0])
    scene = [rectangle(c - 0.5 * a - np.array([0, 0.5, 0]), a, (0.0, 1.0, 0.0))]
    poses, _, out = _two_views(scene, c)
    dist, angle, bound_d, bound_a, held = _surface_errors(out, poses, lambda p: (p - c) @ n, lambda p: np.tile(n, (len(p), 1)), 60.0)
    assert held.sum() > 100
    print("slanted plane: distance max %.3g m (bounds %.3g .. %.3g), angle max %.3g deg (bounds %.3g .. %.3g)"
          % (dist[held].max(), bound_d[held].min(), bound_d[held].max(), angle[held].max(), bound_a[held].min(), bound_a[held].max()))
    assert (dist[held] <= bound_d[held]).all()
    assert (angle[held] <= bound_a[held]).all()


def test_sphere_from_two_views():
    """Measured on the restatement, over the rows both views see within 50 deg of the normal: distance at most 0.31 mm against
    per-row bounds up to 0.73 mm, angle at most 6.0 deg against bounds up to 39 deg; every held row is inside its own bound."""
    c, radius = np.array([0.0, 0.0, 0.43]), 0.04
    poses, _, out = _two_views([sphere(c, radius)], c)

    def normal_of(p):
        d = p - c
        return d / np.linalg.norm(d, axis=1)[:, None]
    dist, angle, bound_d, bound_a, held = _surface_errors(out, poses, lambda p: np.linalg.norm(p - c, axis=1) - radius, normal_of, 50.0)
    assert held.sum() > 50
    print("sphere: distance max %.3g m (bound max %.3g), angle max %.3g deg (bound max %.3g)"
          % (dist[held].max(), bound_d[held].max(), angle[held].max(), bound_a[held].max()))
    assert (dist[held] <= bound_d[held]).all()
    assert (angle[held] <= bound_a[held]).all()


def test_five_noisy_views_average():
    """Five views of one plane, depths offset by known constants: D is the sequential running mean of the five t, recomputed here
    with float32 scalars for one column, and the surface lies at the mean depth: the mean of five linear functions is linear, so
    five times the single-view bound holds, 1.5e-6 m."""
    z0 = 0.4137
    offsets = [0.0011, -0.0007, 0.0004, -0.0013, 0.0009]
    vol = ref.Volume(**SMALL)
    for off in offsets:
        vol.integrate(constant_depth(z0 + off), None, W, H, K)
    assert (vol.W == 5).all()
    centres = vol.centres()
    column = np.arange(vol.n).reshape(20, 20, 20)[:, 7, 11]
    for l in column:
        d, w = f32(1.0), 0
        for off in offsets:
            t = min(f32(f32(f32(z0 + off) - centres[l, 2]) * vol.rtrunc), f32(1.0))
            d = f32(f32(f32(d * f32(w)) + t) / f32(f32(w) + f32(1.0)))
            w += 1
        assert d.view(np.uint32) == vol.D[l].view(np.uint32)
    out = vol.extract()
    k = int(out["num"][0])
    assert k == 400
    mean_depth = np.mean([float(f32(z0 + off)) for off in offsets])
    err = np.abs(out["xyz"][:k, 2].astype(np.float64) - mean_depth).max()
    print("five views: max |z - mean| = %.3g m (bound 1.5e-6)" % err)
    assert err <= 5 * 10 * EPS * 0.5
    assert (out["weight"][:k] == 5).all()


def test_free_space_evidence_removes_a_speckle():
    """View 0 sees a plane at 0.415 m and a speckle of 3 x 3 pixels at 0.395 m; view 1, from the same place, sees the plane alone and so
    looks through the speckle.  View 0 alone leaves the speckle's surface at min_weight = 1: that is all a one-view voxel can say.
    With both views there is none at min_weight = 2 -- and none at min_weight = 1 either: every voxel view 0 made negative (t in
    [-1, 0)) was seen empty by view 1 (t = 1), and the mean of the two is not below 0.  The plane stays."""
    pixel = np.array([v * W + u for v in (23, 24, 25) for u in (32, 33, 34)])      # 3 x 3 pixels: a voxel column surely reads one
    with_speckle, plane = constant_depth(0.415, (pixel, 0.395)), constant_depth(0.415)

    def near_speckle(out):
        k = int(out["num"][0])
        return int((out["xyz"][:k, 2] < 0.405).sum()), k
    alone = ref.Volume(**SMALL)
    alone.integrate(with_speckle, None, W, H, K)
    assert near_speckle(alone.extract())[0] >= 1
    for min_weight in (2, 1):
        vol = ref.Volume(**dict(SMALL, min_weight=min_weight))
        vol.integrate(with_speckle, None, W, H, K)
        counts = vol.integrate(plane, None, W, H, K)
        assert counts[ref.UPDATED] > 0
        speckle_rows, k = near_speckle(vol.extract())
        assert speckle_rows == 0 and k >= 390


def _hand(dims, D, Wt, C=None, **params):
    vol = ref.Volume(**dict(dict(voxel=0.5, trunc=1.0, origin=(0.0, 0.0, 0.0), dims=dims, max_points=64), **params))
    vol.D = np.asarray(D, dtype=np.float32).reshape(-1)
    vol.W = np.asarray(Wt, dtype=np.int32).reshape(-1)
    if C is not None:
        vol.C = np.asarray(C, dtype=np.float32).reshape(-1, 3)
    return vol


def test_max_weight_saturates_into_a_moving_average():
    vol = ref.Volume(**dict(SMALL, max_weight=3))
    depths = [0.4137, 0.4141, 0.4129, 0.4150, 0.4133]
    for z in depths:
        vol.integrate(constant_depth(z), None, W, H, K)
    assert (vol.W == 3).all()
    l = 5 + 20 * (6 + 20 * 17)
    pz = vol.centres()[l, 2]
    t = [float(f32(f32(f32(z) - pz) * vol.rtrunc)) for z in depths]
    assert all(abs(v) < 1 for v in t)
    d = 1.0
    for i, v in enumerate(t):
        w = min(i, 3)
        d = (d * w + v) / (w + 1)                            # in float64: from the fourth view on the old mean counts three times
    assert abs(float(vol.D[l]) - d) <= 16 * EPS


def test_a_voxel_only_seen_as_far_free_space_bounds_no_surface():
    """D = 1 against D < 0: observed, a sign change, and still not a surface."""
    vol = _hand((2, 1, 1), [1.0, -0.5], [4, 4])
    assert vol.extract()["num"].tolist() == [0, 0, 2, 0]
    vol = _hand((2, 1, 1), [np.nextafter(f32(1), f32(0)), -0.5], [4, 4])
    assert vol.extract()["num"].tolist() == [1, 1, 2, 0]


def test_keys_ascend_and_overflow_keeps_the_smallest():
    """A 3 x 3 x 3 checkerboard of +-0.5: every inside neighbour pair is a crossing, 54 candidates; the rows are sorted by 3 l + a."""
    ix, iy, iz = np.meshgrid(np.arange(3), np.arange(3), np.arange(3), indexing="ij")
    D = np.where((ix + iy + iz) % 2 == 0, 0.5, -0.5).transpose(2, 1, 0)          # [iz, iy, ix]
    vol = _hand((3, 3, 3), D, np.full(27, 2))
    full = vol.extract()
    assert full["num"].tolist() == [54, 54, 27, 0]
    assert (np.diff(full["keys"]) > 0).all()
    assert full["keys"][:3].tolist() == [0, 1, 2]            # voxel 0 crosses on all three axes
    assert np.allclose(full["xyz"][0], [0.5, 0.25, 0.25]) and np.allclose(full["xyz"][1], [0.25, 0.5, 0.25])
    few = _hand((3, 3, 3), D, np.full(27, 2), max_points=10).extract()
    assert few["num"].tolist() == [10, 54, 27, 1]
    assert (few["keys"] == full["keys"][:10]).all()
    assert (few["xyz"].view(np.uint32) == full["xyz"][:10].view(np.uint32)).all()


@pytest.mark.parametrize("bad", [dict(voxel=0.0), dict(trunc=0.003), dict(dims=(0, 1, 1)), dict(max_points=(1 << 21) + 1),
                                 dict(min_weight=0), dict(origin=(0.0, 1.0))])
def test_params_are_validated(bad):
    """``TsdfParams`` needs only the header and no device; the module imports the library, which the build leaves in the tree."""
    with pytest.raises(ValueError):
        tsdf.TsdfParams(**bad)
    assert tsdf.TsdfParams().dims == (320, 320, 320) and tsdf.TsdfParams.coerce({"voxel": 0.004}).voxel == 0.004


def test_the_restatement_has_the_products_defaults():
    import dataclasses
    assert ref.DEFAULTS == dataclasses.asdict(tsdf.TsdfParams())
    assert (ref.UPDATED, ref.NOT_IN_VIEW, ref.NO_DEPTH, ref.BEHIND) == (tsdf.UPDATED, tsdf.NOT_IN_VIEW, tsdf.NO_DEPTH, tsdf.BEHIND)
    assert np.array_equal(ref.camera_from_common(None), tsdf.camera_from_common(None))
