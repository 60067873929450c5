"""The distance field of the TSDF volume on the MI355X (csrc/edt.hip through tsdf.Volume.distance_field, DistanceField.query and
approach.analyse_volume(field=...)) against the all-pairs numpy restatement (tests/edt_reference.py).  Every comparison is bit
for bit: squared distances and indices are integers, the query's metres are one exact conversion, one correctly rounded root and
one product.  Volumes are set by hand through ``Volume.D`` / ``Volume.W``."""
import functools

import numpy as np
import pytest
import torch

from . import approach_reference as cloud_ref
from . import approach_volume_reference as av_ref
from . import edt_reference as ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
f32 = np.float32
NONE = ref.NONE
SENTINEL = -77
GUARD = 64                                   # sentinel words on either side of an output plane
DYADIC_BOX = (-0.5, 0.5, 0.125, 1.0, 0.75, 0.0)
IDENTITY_L = np.eye(4, dtype=np.float32)[:3].reshape(1, 12)
TURNED = np.array([[0.36, 0.48, -0.8, 0.01], [-0.8, 0.6, 0.0, -0.02], [0.48, 0.64, 0.6, 0.015], [0, 0, 0, 1.0]])   # a rotation


def _dev(a, dtype=np.float32):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(DEV)


def _hand(dims, mask=None, origin=(-1.0, -1.0, -0.5), voxel=0.25, trunc=1.0, min_weight=1):
    """A hand-set volume: observed free (D = 1, W = min_weight) with D = -0.5 where ``mask`` is set."""
    hand = av_ref.HandVolume(dims, origin, voxel, trunc=trunc, min_weight=min_weight).observe_all(1.0, min_weight)
    if mask is not None:
        hand.D[np.asarray(mask, dtype=bool)] = f32(-0.5)
    return hand


def _volume(hand):
    from regnet_for_3d_grasping_amd import tsdf
    vol = tsdf.Volume(tsdf.TsdfParams(voxel=hand.voxel, trunc=hand.trunc, origin=tuple(float(v) for v in hand.origin), dims=hand.dims,
                                      min_weight=hand.min_weight, max_points=1 << 10), DEV)
    vol.D.copy_(_dev(hand.D))
    vol.W.copy_(_dev(hand.W, np.int32))
    return vol


def _kernel(vol, mode=0, outside=0, nearest=True, margin=0.0, min_weight=None, stream=None):
    """regnet_tsdf_edt on a ``tsdf.Volume`` -> (dist2, nearest or None) as numpy arrays, written into the middle of guarded
    buffers whose sentinel words must survive."""
    from regnet_for_3d_grasping_amd import _lib
    p = vol.params
    n = p.dims[0] * p.dims[1] * p.dims[2]
    planes = [torch.full((n + 2 * GUARD,), SENTINEL, dtype=torch.int32, device=DEV) for _ in range(2 if nearest else 1)]
    _lib.call("regnet_tsdf_edt", vol.data, vol.data.data_ptr(), *p.dims, float(p.trunc),
              int(p.min_weight if min_weight is None else min_weight), float(margin), int(mode), int(outside),
              planes[0][GUARD:].data_ptr(), planes[1][GUARD:].data_ptr() if nearest else None, stream=stream)
    out = [t.cpu().numpy() for t in planes]
    for a in out:
        assert (a[:GUARD] == SENTINEL).all() and (a[-GUARD:] == SENTINEL).all()
    return out[0][GUARD:-GUARD], (out[1][GUARD:-GUARD] if nearest else None)


def _check_mask(dims, mask, outside=0, what=""):
    """Device and restatement on the volume whose SOLID voxels are ``mask`` -> (dist2, nearest)."""
    mask = np.asarray(mask, dtype=bool)
    got = _kernel(_volume(_hand(dims, mask)), 0, outside)
    want = ref.transform(mask, dims, bool(outside))
    assert got[0].dtype == np.int32 and got[1].dtype == np.int32
    assert np.array_equal(got[0], want[0]), (what, dims, outside, np.flatnonzero(got[0] != want[0])[:8])
    assert np.array_equal(got[1], want[1]), (what, dims, outside, np.flatnonzero(got[1] != want[1])[:8])
    return got


def _at(dims, ix, iy, iz):
    return (iz * dims[1] + iy) * dims[0] + ix


def _mask(dims, voxels):
    m = np.zeros((dims[0] * dims[1] * dims[2],), dtype=bool)
    for v in voxels:
        m[_at(dims, *v)] = True
    return m


def _random_mask(dims, density, seed=0):
    n = dims[0] * dims[1] * dims[2]
    mask = np.random.default_rng(seed + n).random(n) < density
    if not mask.any():
        mask[n // 2] = True
    return mask


# ---- ragged dims ----------------------------------------------------------------------------------------------------------------
RAGGED = [(1, 1, 1), (1, 1, 7), (5, 1, 3), (67, 3, 5), (3, 67, 5), (3, 5, 67), (130, 70, 9), (300, 2, 3), (2, 300, 3), (3, 2, 300),
          (1024, 1, 2), (1, 1024, 2), (2, 1, 1024)]


@pytest.mark.parametrize("dims", RAGGED, ids=lambda d: "%dx%dx%d" % d)
def test_ragged_dims(dims):
    density = 0.01 if dims == (130, 70, 9) else 0.05      # (the all-pairs restatement is what takes the time)
    mask = _random_mask(dims, density)
    _check_mask(dims, mask, 0)
    _check_mask(dims, mask, 1)


# ---- masks ----------------------------------------------------------------------------------------------------------------------
MID = (37, 19, 11)


def test_no_obstacle_and_every_voxel_an_obstacle():
    n = MID[0] * MID[1] * MID[2]
    d2, near = _check_mask(MID, np.zeros((n,), dtype=bool))
    assert (d2 == NONE).all() and (near == -1).all()
    d2, near = _check_mask(MID, np.zeros((n,), dtype=bool), outside=1)
    assert d2.max() == 36 and (near == -1).all()
    d2, near = _check_mask(MID, np.ones((n,), dtype=bool))
    assert (d2 == 0).all() and np.array_equal(near, np.arange(n))
    _check_mask(MID, np.ones((n,), dtype=bool), outside=1)


def test_the_eight_corners():
    corners = [(x, y, z) for x in (0, MID[0] - 1) for y in (0, MID[1] - 1) for z in (0, MID[2] - 1)]
    d2, near = _check_mask(MID, _mask(MID, corners))
    assert d2[_at(MID, 18, 9, 5)] == 18 * 18 + 9 * 9 + 5 * 5 and near[_at(MID, 18, 9, 5)] == 0      # an eight-way tie: index 0
    _check_mask(MID, _mask(MID, corners), outside=1)


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_one_obstacle_at_the_far_end_of_a_300_line(axis):
    dims = [3, 2, 3]
    dims[axis] = 300
    dims = tuple(dims)
    far = [1, 1, 1]
    far[axis] = 299
    d2, near = _check_mask(dims, _mask(dims, [far]))
    near_end = list(far)
    near_end[axis] = 0
    assert d2[_at(dims, *near_end)] == 299 * 299 and (near == _at(dims, *far)).all()


@pytest.mark.parametrize("density", [0.001, 0.05, 0.5])
def test_seeded_random_masks(density):
    mask = _random_mask(MID, density, seed=int(density * 1000))
    _check_mask(MID, mask, 0)
    _check_mask(MID, mask, 1)


def test_the_six_neighbour_tie_and_single_axis_ties():
    dims = (3, 3, 3)
    faces = [(0, 1, 1), (2, 1, 1), (1, 0, 1), (1, 2, 1), (1, 1, 0), (1, 1, 2)]
    d2, near = _check_mask(dims, _mask(dims, faces))
    assert d2[_at(dims, 1, 1, 1)] == 1 and near[_at(dims, 1, 1, 1)] == _at(dims, 1, 1, 0)
    for axis in range(3):
        dims = [3, 3, 3]
        dims[axis] = 9
        lo, hi, mid = [1, 1, 1], [1, 1, 1], [1, 1, 1]
        lo[axis], hi[axis], mid[axis] = 2, 6, 4
        d2, near = _check_mask(tuple(dims), _mask(dims, [lo, hi]))
        assert d2[_at(dims, *mid)] == 4 and near[_at(dims, *mid)] == _at(dims, *lo)
    # unequal terms that tie: (dx, dy) = (0, 5) against (3, 4) and (4, 3), on either side
    dims = (11, 11, 1)
    d2, near = _check_mask(dims, _mask(dims, [(5, 10, 0), (8, 1, 0), (1, 2, 0)]))
    assert d2[_at(dims, 5, 5, 0)] == 25 and near[_at(dims, 5, 5, 0)] == _at(dims, 8, 1, 0)


def test_a_tie_across_a_tile_boundary_of_the_y_and_z_passes():
    """The y / z passes stage ``regnet_edt_tile`` consecutive ix per workgroup: ties whose two obstacles lie in different tiles,
    and ties along y and z in the last column of one tile and the first of the next."""
    from regnet_for_3d_grasping_amd import _lib
    dims = (130, 70, 9)
    tiles = {int(_lib.lib.regnet_edt_tile(n, w)) for n in dims[1:] for w in (0, 1)}
    assert tiles <= {8, 16, 32, 64} and all(t < dims[0] for t in tiles)
    voxels = []
    for t in sorted(tiles | {8, 16, 32, 64}):
        voxels += [(t - 2, 5, 1), (t + 2, 5, 1)]                                   # a tie along x at ix = t, across the boundary
        voxels += [(t - 1, 30, 4), (t - 1, 40, 4), (t, 30, 4), (t, 40, 4)]         # ties along y at iy = 35 in both columns
        voxels += [(t - 1, 60, 2), (t - 1, 60, 8), (t, 60, 2), (t, 60, 8)]         # ties along z at iz = 5 in both columns
    mask = _mask(dims, voxels)
    for nearest in (True, False):
        got = _kernel(_volume(_hand(dims, mask)), 0, 0, nearest=nearest)
        want = _reference_tiles(mask.tobytes(), dims)
        assert np.array_equal(got[0], want[0])
        if nearest:
            assert np.array_equal(got[1], want[1])
            assert got[1][_at(dims, 64, 5, 1)] == _at(dims, 62, 5, 1) and got[1][_at(dims, 64, 35, 4)] == _at(dims, 64, 30, 4)


@functools.lru_cache(maxsize=None)
def _reference_tiles(mask_bytes, dims):
    return ref.transform(np.frombuffer(mask_bytes, dtype=bool), dims)


# ---- classification -------------------------------------------------------------------------------------------------------------
def test_classification_weights_thresholds_nan_modes_and_the_outside():
    dims, trunc, margin, min_weight = (9, 1, 1), 0.75, 0.1, 3
    d_solid = f32(margin / trunc)
    hand = av_ref.HandVolume(dims, (-1.0, -1.0, -0.5), 0.25, trunc=trunc, min_weight=min_weight).observe_all(1.0, min_weight)
    hand.D[1], hand.W[1] = -0.5, min_weight                         # SOLID at exactly min_weight
    hand.D[2], hand.W[2] = -0.5, min_weight - 1                     # one below: UNKNOWN
    hand.D[3] = np.nextafter(d_solid, f32(-1))                      # one ulp below d_solid: SOLID
    hand.D[4] = d_solid                                             # at d_solid: FREE (strict)
    hand.D[5] = np.nextafter(d_solid, f32(1))                       # one ulp above: FREE
    hand.D[6] = np.nan                                              # UNKNOWN
    vol = _volume(hand)
    for mode in (0, 1):
        for outside in (0, 1):
            got = _kernel(vol, mode, outside, margin=margin)
            want = ref.edt_ref(hand.D, hand.W, dims, trunc, min_weight, margin, mode, outside)
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), (mode, outside)
            zero = (got[0] == 0).tolist()
            assert zero == [False, True, mode == 1, True, False, False, mode == 1, False, False], (mode, outside, zero)
    d2, near = _kernel(vol, 0, 0, margin=margin)
    assert d2.tolist() == [1, 0, 1, 0, 1, 4, 9, 16, 25] and near.tolist() == [1, 1, 1, 3, 3, 3, 3, 3, 3]
    # min_weight given to the call, not the volume's
    got = _kernel(vol, 1, 0, margin=margin, min_weight=2)
    want = ref.edt_ref(hand.D, hand.W, dims, trunc, 2, margin, 1, 0)
    assert np.array_equal(got[0], want[0]) and got[0][2] == 0 and np.array_equal(got[1], want[1])


def test_a_face_tie_goes_to_the_interior_obstacle():
    dims = (5, 5, 5)
    d2, near = _check_mask(dims, _mask(dims, [(2, 2, 3)]), outside=1)
    assert d2[_at(dims, 2, 2, 1)] == 4 and near[_at(dims, 2, 2, 1)] == _at(dims, 2, 2, 3)       # 2 from the obstacle and from z = -1
    assert d2[_at(dims, 2, 2, 0)] == 1 and near[_at(dims, 2, 2, 0)] == -1                       # the outside is strictly nearer


# ---- the Python layer, streams, graphs, repeatability ---------------------------------------------------------------------------
def test_distance_field_nearest_null_side_stream_graph_replay_and_two_runs():
    from regnet_for_3d_grasping_amd import tsdf
    dims = (67, 21, 13)
    masks = [_random_mask(dims, 0.01, seed=s) for s in (1, 2)]
    hands = [_hand(dims, m, min_weight=2) for m in masks]
    hands[0].W[::7] = 1                                              # unobserved speckles: the modes differ
    vol = _volume(hands[0])
    want = ref.edt_ref(hands[0].D, hands[0].W, dims, 1.0, 2, 0.0, 1, True)
    field = vol.distance_field("solid_or_unseen", nearest=True)
    assert isinstance(field, tsdf.DistanceField) and field.outside and field.mode == "solid_or_unseen" and field.dims == dims
    assert field.bytes() == 8 * dims[0] * dims[1] * dims[2] and field.dist2.dtype == torch.int32
    assert np.array_equal(field.dist2.cpu().numpy(), want[0]) and np.array_equal(field.nearest.cpu().numpy(), want[1])
    plain = vol.distance_field("solid_or_unseen")                   # nearest = NULL: the same dist2 bytes
    assert plain.nearest is None and plain.bytes() == 4 * field.dist2.numel() and torch.equal(plain.dist2, field.dist2)
    solid = vol.distance_field("solid", nearest=True)
    assert not solid.outside
    want_solid = ref.edt_ref(hands[0].D, hands[0].W, dims, 1.0, 2, 0.0, 0, False)
    assert np.array_equal(solid.dist2.cpu().numpy(), want_solid[0]) and np.array_equal(solid.nearest.cpu().numpy(), want_solid[1])
    assert torch.equal(vol.distance_field("solid", outside=True, min_weight=1).dist2,
                       _dev(ref.edt_ref(hands[0].D, hands[0].W, dims, 1.0, 1, 0.0, 0, True)[0], np.int32))
    metres = field.metres()
    assert metres.dtype == torch.float32 and metres.cpu().numpy().tobytes() == ref.metres_ref(want[0], 0.25).tobytes()
    with pytest.raises(ValueError):
        vol.distance_field("unseen")
    # a side stream, twice, into the same buffers (out=)
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    again = vol.distance_field("solid_or_unseen", nearest=True, stream=side)
    reused = vol.distance_field("solid_or_unseen", nearest=True, stream=side, out=again)
    side.synchronize()
    torch.cuda.current_stream(DEV).wait_stream(side)
    assert reused is again and torch.equal(again.dist2, field.dist2) and torch.equal(again.nearest, field.nearest)
    # captured and replayed on another volume state
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        vol.distance_field("solid_or_unseen", nearest=True, out=again)
    for k in (1, 0):
        vol.D.copy_(_dev(hands[k].D))
        vol.W.copy_(_dev(hands[k].W, np.int32))
        again.dist2.fill_(SENTINEL)
        again.nearest.fill_(SENTINEL)
        graph.replay()
        torch.cuda.synchronize()
        w = ref.edt_ref(hands[k].D, hands[k].W, dims, 1.0, 2, 0.0, 1, True)
        assert np.array_equal(again.dist2.cpu().numpy(), w[0]) and np.array_equal(again.nearest.cpu().numpy(), w[1]), k


def test_every_error_code_of_the_transform_leaves_the_outputs_alone():
    from regnet_for_3d_grasping_amd import _lib
    vol = _volume(_hand((6, 8, 2), _mask((6, 8, 2), [(1, 2, 0)])))
    d2 = torch.full((96,), SENTINEL, dtype=torch.int32, device=DEV)
    near = torch.full((96,), SENTINEL, dtype=torch.int32, device=DEV)
    stream = torch.cuda.current_stream(DEV).cuda_stream

    def raw(volume=vol.data.data_ptr(), dims=(6, 8, 2), trunc=1.0, min_weight=1, margin=0.0, mode=0, outside=0, d=d2.data_ptr(),
            n=near.data_ptr()):
        return _lib.lib.regnet_tsdf_edt(volume, dims[0], dims[1], dims[2], trunc, min_weight, margin, mode, outside, d, n, stream)

    assert raw(dims=(0, 8, 2)) == -1 and raw(dims=(6, 8, -1)) == -1 and raw(min_weight=0) == -1
    assert raw(mode=2) == -1 and raw(mode=-1) == -1 and raw(outside=2) == -1 and raw(outside=-1) == -1
    assert raw(dims=(1025, 1, 1)) == -3 and raw(dims=(1, 1, 1025)) == -3 and raw(dims=(1024, 1024, 512)) == -3
    for name in ("trunc", "margin"):
        for bad in (float("nan"), float("inf"), 1e300):
            assert raw(**{name: bad}) == -3, (name, bad)
    assert raw(trunc=0.0) == -3
    assert raw(volume=None) == -2 and raw(d=None) == -2
    assert _lib.lib.regnet_tsdf_edt_pass(vol.data.data_ptr(), 6, 8, 2, 1.0, 1, 0.0, 0, 0, 3, d2.data_ptr(), None, stream) == -1
    torch.cuda.synchronize()
    assert (d2 == SENTINEL).all() and (near == SENTINEL).all()
    assert raw() == 0 and raw(n=None) == 0
    torch.cuda.synchronize()
    want = ref.transform(_mask((6, 8, 2), [(1, 2, 0)]), (6, 8, 2))
    assert np.array_equal(d2.cpu().numpy(), want[0]) and np.array_equal(near.cpu().numpy(), want[1])


# ---- the query ------------------------------------------------------------------------------------------------------------------
QDIMS, QORIGIN, QVOXEL = (9, 7, 5), (-1.0, -1.0, -0.5), 0.25


@functools.lru_cache(maxsize=None)
def _query_field():
    mask = _random_mask(QDIMS, 0.03, seed=5)
    vol = _volume(_hand(QDIMS, mask, QORIGIN, QVOXEL))
    return vol.distance_field("solid", nearest=True), ref.transform(mask, QDIMS)


def _query_and_check(field, want, points, to_volume=None, nearest=True):
    got = field.query(points, to_volume, nearest=nearest)
    rows = np.eye(4)[:3].reshape(12) if to_volume is None else np.asarray(to_volume, dtype=np.float64)[:3].reshape(12)
    distance, xyz = ref.query_ref(want[0], want[1] if field.has_nearest else None, field.dims, field.origin, field.voxel,
                                  points.cpu().numpy(), rows.astype(np.float32))
    d = (got[0] if nearest else got).cpu().numpy()
    assert d.dtype == np.float32 and d.tobytes() == distance.tobytes(), (d, distance)
    if nearest:
        assert got[1].cpu().numpy().tobytes() == xyz.tobytes()
    return distance, xyz


def test_query_faces_ulps_nan_rows_strides_and_a_transform():
    field, want = _query_field()
    lo = np.asarray(QORIGIN, dtype=np.float32)
    hi = (lo + np.asarray(QDIMS, dtype=np.float32) * f32(QVOXEL)).astype(np.float32)
    rows = [[lo[0] + f32(QVOXEL) * i, lo[1] + f32(QVOXEL) * j, lo[2] + f32(QVOXEL) * k]       # on exact voxel faces
            for i in range(QDIMS[0] + 1) for j in (0, 3, QDIMS[1]) for k in (0, 2, QDIMS[2])]
    inner = [0.1, 0.1, 0.1]
    for axis in range(3):                                           # one ulp inside and outside each face of the volume
        for face, towards in ((lo, -np.inf), (hi, np.inf)):
            for sign in (1, -1):
                p = list(inner)
                p[axis] = np.nextafter(face[axis], f32(towards * sign))
                rows.append(p)
            p = list(inner)
            p[axis] = face[axis]
            rows.append(p)
    rows += [[np.nan, 0, 0], [0, np.nan, 0], [0, 0, np.nan], [np.inf, 0, 0], [0, -np.inf, 0]]
    rng = np.random.default_rng(3)
    rows += rng.uniform(-1.3, 1.5, (200, 3)).tolist()
    points = _dev(np.asarray(rows, dtype=np.float32))
    distance, xyz = _query_and_check(field, want, points)
    assert np.isnan(distance).any() and np.isfinite(distance).any() and np.isfinite(xyz).any()
    assert np.isnan(distance[-205:-200]).all()
    _query_and_check(field, want, points, nearest=False)
    _query_and_check(field, want, points, TURNED)
    wide = torch.zeros((points.shape[0], 7), device=DEV)
    wide[:, 1:6:2] = points
    _query_and_check(field, want, wide[:, 1:6:2])                   # strided columns
    _query_and_check(field, want, points.t().contiguous().t())      # column-major rows


@pytest.mark.parametrize("M", [0, 1, 63, 64, 65])
def test_query_sizes(M):
    field, want = _query_field()
    points = _dev(np.random.default_rng(M).uniform(-1.0, 0.7, (M, 3)).astype(np.float32).reshape(M, 3))
    distance, _ = _query_and_check(field, want, points)
    assert distance.shape == (M,)


def test_query_of_an_empty_field_and_of_one_without_nearest():
    vol = _volume(_hand(QDIMS, None, QORIGIN, QVOXEL))
    field = vol.distance_field("solid", nearest=True)
    points = _dev(np.array([[0.1, 0.1, 0.1], [5.0, 0, 0]], dtype=np.float32))
    d, xyz = field.query(points, nearest=True)
    assert d.cpu().numpy().tobytes() == np.array([np.inf, np.nan], dtype=np.float32).tobytes() and torch.isnan(xyz).all()
    assert (field.metres() == float("inf")).all()
    plain = vol.distance_field("solid")
    with pytest.raises(ValueError):
        plain.query(points, nearest=True)
    assert plain.query(points).cpu().numpy().tobytes() == d.cpu().numpy().tobytes()


# ---- the margin -----------------------------------------------------------------------------------------------------------------
# The dyadic box of tests/test_gpu_approach_volume.py: S = 0.5, h = voxel = 0.25; under the identity the 6 x 8 x 1 samples
# (x = -0.875 .. 0.375, y = -0.875 .. 0.875, z = 0) are voxel centres of a 12 x 12 x 1 volume with origin (-1.5, -1.5, -0.125).
MDIMS, MORIGIN = (12, 12, 1), (-1.5, -1.5, -0.125)


def _mv(x, y):
    return (int((x + 1.5) / 0.25), int((y + 1.5) / 0.25), 0)


def _margin_kernel(dist2, dims, origin, voxel, outside, L, box, standoff, step, x_extent):
    from regnet_for_3d_grasping_amd import _lib
    L = _dev(L)
    B = int(L.shape[0])
    x_lo, x_hi, ht, hw, hs, back_x = box
    per = _dev(x_hi) if np.ndim(x_hi) else None
    origin = np.ascontiguousarray(np.asarray(origin, dtype=np.float32))
    margins = torch.full((B + 2, 2), SENTINEL, dtype=torch.int32, device=DEV)
    counts = torch.full((B + 2, 4), SENTINEL, dtype=torch.int32, device=DEV)
    d2 = _dev(dist2, np.int32)
    _lib.call("regnet_grasp_margin_volume_f32", d2, d2.data_ptr(), *dims, origin.ctypes.data, float(voxel), int(outside), L.data_ptr(),
              B, float(x_lo), 0.0 if per is not None else float(x_hi), None if per is None else per.data_ptr(), float(ht), float(hw),
              float(hs), float(back_x), float(standoff), float(step), float(x_extent), margins[1:].data_ptr(), counts[1:].data_ptr())
    margins, counts = margins.cpu().numpy(), counts.cpu().numpy()
    assert (margins[[0, -1]] == SENTINEL).all() and (counts[[0, -1]] == SENTINEL).all()
    return margins[1:-1], counts[1:-1]


def _margin_both(dist2, dims, origin, voxel, outside, L, box, standoff, step, x_extent):
    got = _margin_kernel(dist2, dims, origin, voxel, outside, L, box, standoff, step, x_extent)
    want = ref.margin_ref(dist2, dims, origin, voxel, outside, L, box, standoff, step, x_extent)
    assert np.array_equal(got[0], want[0]), (got[0], want[0])
    assert np.array_equal(got[1], want[1]), (got[1], want[1])
    return got


def _dyadic_margin(obstacles, outside=0, L=IDENTITY_L, box=DYADIC_BOX, x_extent=0.5):
    mask = _mask(MDIMS, obstacles)
    dist2, _ = _kernel(_volume(_hand(MDIMS, mask, MORIGIN, 0.25)), 0, outside)
    assert np.array_equal(dist2, ref.transform(mask, MDIMS, bool(outside))[0])
    margins, counts = _margin_both(dist2, MDIMS, MORIGIN, 0.25, outside, L, box, 0.5, 0.25, x_extent)
    return margins[0].tolist(), counts[0].tolist()


def test_margin_rules_on_hand_set_volumes():
    # 16 back + 8 finger samples, 4 of them both: 20 hand samples; 24 inner blockers (x < 0) + 12 in the lanes (x < 0.5), which
    # hold every hand sample: 36 swept samples
    assert _dyadic_margin([]) == ([NONE, NONE], [20, 0, 36, 0])
    # beyond a finger tip: two voxels from the finger sample (0.375, 0.875) alone
    assert _dyadic_margin([_mv(0.875, 0.875)])[0] == [4, 4]
    # behind the hand: two voxels from the blocker (-0.875, 0.125), four from the back samples
    assert _dyadic_margin([_mv(-1.375, 0.125)])[0] == [16, 4]
    # between the fingers, in the closing region, which is not part of the hand: two voxels from the palm (-0.125, 0.125)
    assert _dyadic_margin([_mv(0.375, 0.125)])[0] == [4, 4]
    # in a hand sample's own voxel
    assert _dyadic_margin([_mv(-0.375, 0.375)])[0] == [0, 0]
    # per-grasp x_hi: the fingers of the second grasp end at 0.25, so the obstacle beyond the tip is further from them
    L2 = np.repeat(IDENTITY_L, 2, axis=0)
    mask = _mask(MDIMS, [_mv(0.875, 0.875)])
    dist2 = ref.transform(mask, MDIMS)[0]
    box = (-0.5, np.array([0.5, 0.25], dtype=np.float32), 0.125, 1.0, 0.75, 0.0)
    margins, counts = _margin_both(dist2, MDIMS, MORIGIN, 0.25, 0, L2, box, 0.5, 0.25, 0.5)
    assert margins.tolist() == [[4, 4], [9, 9]] and counts.tolist() == [[20, 0, 36, 0], [18, 0, 34, 0]]


def test_margin_outside_samples_nan_rows_and_no_grasp():
    # the hand moved so that its far lane leaves the volume: x + 1.25 puts x = 0.375 at 1.625 > 1.5
    L = IDENTITY_L.copy()
    L[0, 3] = 1.25
    for outside in (0, 1):
        margins, counts = _dyadic_margin([_mv(-1.375, -1.375)], outside, L)
        assert counts == [20, 2, 36, 2]
        assert margins == ([0, 0] if outside else [85, 53])
    bad = np.repeat(IDENTITY_L, 3, axis=0)
    bad[1, 5] = np.nan
    dist2 = ref.transform(_mask(MDIMS, [_mv(0.875, 0.875)]), MDIMS)[0]
    for outside in (0, 1):
        margins, counts = _margin_both(dist2, MDIMS, MORIGIN, 0.25, outside, bad, DYADIC_BOX, 0.5, 0.25, 0.5)
        assert counts[1].tolist() == [20, 20, 36, 36] and margins[1].tolist() == ([0, 0] if outside else [NONE, NONE])
        assert margins[0].tolist() == [4, 4] and margins[2].tolist() == [4, 4]
    margins, counts = _margin_kernel(dist2, MDIMS, MORIGIN, 0.25, 0, np.zeros((0, 12), dtype=np.float32), DYADIC_BOX, 0.5, 0.25, 0.5)
    assert margins.shape == (0, 2) and counts.shape == (0, 4)


GRIPPER = av_ref.gripper_box(0.06, 0.08)
FINE = ((40, 36, 33), (-0.1, -0.09, -0.08), 0.005)


@pytest.mark.parametrize("i,j", [(0, 0), (9, 3), (17, 1), (27, 1), (12, 1), (20, 19), (27, 19)])
def test_the_deciding_sample_of_the_margin_is_found_in_every_wave(i, j):
    """The reference's gripper at a 5 mm step with a 2 cm standoff: 28 x 21 x 2 samples, 4 x 3 tiles of 8 x 8, tile t = 4 ty + tx on
    wave t % 4, the last row and column of tiles partial.  The field is 1000 everywhere but 7 in the voxel of the swept sample
    (i, j, 1): one per wave in the first row of tiles, the partial tile of the first row, and the last row with its partial tile."""
    dims, origin, voxel = FINE
    xv, yv, zv = av_ref.lattice_samples(GRIPPER, 0.02, voxel, 0.06)
    assert (len(xv), len(yv), len(zv)) == (28, 21, 2)
    inside, v = ref.lookup(np.array([[xv[i], yv[j], zv[1]]], dtype=np.float32), IDENTITY_L[0], dims, origin, voxel)
    assert inside[0]
    dist2 = np.full((dims[0] * dims[1] * dims[2],), 1000, dtype=np.int32)
    dist2[v[0]] = 7
    margins, _ = _margin_both(dist2, dims, origin, voxel, 0, IDENTITY_L, GRIPPER, 0.02, voxel, 0.06)
    assert margins[0, 1] == 7 and margins[0, 0] in (7, 1000)


@functools.lru_cache(maxsize=None)
def _fine_volume():
    dims, origin, voxel = FINE
    mask = _random_mask(dims, 0.0005, seed=11)
    hand = _hand(dims, mask, origin, voxel, trunc=0.02, min_weight=2)
    n = hand.D.shape[0]
    hand.W[(np.arange(n) % dims[0]) >= 39] = 1                      # a never-observed layer (thin: the restatement is all pairs)
    return hand, _volume(hand)


def test_analyse_volume_with_a_field_per_grasp_depths_and_unchanged_outputs():
    from regnet_for_3d_grasping_amd import approach
    hand, vol = _fine_volume()
    dims, origin, voxel = FINE
    B = 67
    grasp = _dev(cloud_ref.random_grasps(np.random.default_rng(B), B, spread=0.05))
    per = _dev(np.random.default_rng(B).uniform(0.03, 0.08, B))
    for unseen, depth, max_depth in (("free", 0.06, None), ("blocked", per, 0.08)):
        blocked = unseen == "blocked"
        params = approach.ApproachParams(space="volume", standoff=0.05, step=0.004, unseen=unseen, field=True, min_margin=0.012)
        field = vol.distance_field("solid_or_unseen" if blocked else "solid")
        want_d2 = ref.edt_ref(hand.D, hand.W, dims, 0.02, 2, 0.0, int(blocked), blocked)[0]
        assert np.array_equal(field.dist2.cpu().numpy(), want_d2)
        res = approach.analyse_volume(vol, grasp, depth, 0.08, params, to_volume=TURNED, max_depth=max_depth, field=field)
        plain_params = approach.ApproachParams(space="volume", standoff=0.05, step=0.004, unseen=unseen)
        plain = approach.analyse_volume(vol, grasp, depth, 0.08, plain_params, to_volume=TURNED, max_depth=max_depth)
        assert plain.margin_hand is None and plain.margins is None
        for name in ("counts", "values", "L", "clearance", "width", "offset", "opening", "pregrasp", "unseen_share", "solid_hand"):
            assert getattr(res, name).cpu().numpy().tobytes() == getattr(plain, name).cpu().numpy().tobytes(), name
        host_depth = depth.cpu().numpy() if isinstance(depth, torch.Tensor) else depth
        box = av_ref.gripper_box(host_depth, 0.08)
        want = ref.margin_ref(want_d2, dims, origin, voxel, int(blocked), res.L.cpu().numpy(), box, 0.05, 0.004,
                              max_depth if max_depth is not None else depth)
        assert np.array_equal(res.margins.cpu().numpy(), want[0]) and np.array_equal(res.margin_counts.cpu().numpy(), want[1])
        assert res.margin_hand.dtype == torch.float32 and res.margin_hand.shape == (B,)
        assert res.margin_hand.cpu().numpy().tobytes() == ref.metres_ref(want[0][:, 0], voxel).tobytes()
        assert res.margin_sweep.cpu().numpy().tobytes() == ref.metres_ref(want[0][:, 1], voxel).tobytes()
        assert (want[0][:, 1] <= want[0][:, 0]).all()
        if not blocked:                               # not vacuous: many different margins, on either side of min_margin
            assert len(np.unique(want[0][:, 0])) > 5
        keep = ref.metres_ref(want[0][:, 0], voxel) >= f32(0.012)
        assert np.array_equal(res.passes().cpu().numpy(), plain.passes().cpu().numpy() & keep) and keep.any() and not keep.all()
    with pytest.raises(ValueError):
        approach.analyse_volume(vol, grasp, 0.06, 0.08, approach.ApproachParams(space="volume", field=True, min_margin=0.01)).passes()


def test_every_error_code_of_the_query_and_the_margin():
    from regnet_for_3d_grasping_amd import _lib
    field, _ = _query_field()
    points = _dev(np.zeros((4, 3), dtype=np.float32))
    out = torch.full((4,), float(SENTINEL), dtype=torch.float32, device=DEV)
    rows = np.ascontiguousarray(np.eye(4, dtype=np.float32)[:3].reshape(12))
    stream = torch.cuda.current_stream(DEV).cuda_stream

    def query(d=field.dist2.data_ptr(), dims=QDIMS, origin3=field.origin.ctypes.data, voxel=QVOXEL, p=points.data_ptr(), M=4,
              t=rows.ctypes.data, o=out.data_ptr()):
        return _lib.lib.regnet_edt_query_f32(d, None, dims[0], dims[1], dims[2], origin3, voxel, p, 3, 1, M, t, o, None, stream)

    assert query(M=-1) == -1 and query(dims=(0, 7, 5)) == -1
    assert query(dims=(1025, 7, 5)) == -3 and query(M=1 << 31) == -3
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        assert query(voxel=bad) == -3
    for null in ("d", "origin3", "p", "t", "o"):
        assert query(**{null: None}) == -2, null
    assert query(M=0) == 0 and query(M=0, d=None) == 0
    m = torch.full((2, 2), SENTINEL, dtype=torch.int32, device=DEV)
    c = torch.full((2, 4), SENTINEL, dtype=torch.int32, device=DEV)
    d2 = _dev(np.zeros((144,), dtype=np.int32), np.int32)
    L = _dev(np.repeat(IDENTITY_L, 2, axis=0))
    origin = np.ascontiguousarray(np.asarray(MORIGIN, dtype=np.float32))

    def margin(d=d2.data_ptr(), dims=MDIMS, origin3=origin.ctypes.data, voxel=0.25, outside=0, l=L.data_ptr(), B=2, standoff=0.5,
               step=0.25, x_extent=0.5, mm=m.data_ptr(), cc=c.data_ptr()):
        return _lib.lib.regnet_grasp_margin_volume_f32(d, dims[0], dims[1], dims[2], origin3, voxel, outside, l, B, -0.5, 0.5, None,
                                                       0.125, 1.0, 0.75, 0.0, standoff, step, x_extent, mm, cc, stream)

    assert margin(B=-1) == -1 and margin(dims=(12, 0, 1)) == -1 and margin(outside=2) == -1 and margin(outside=-1) == -1
    assert margin(dims=(1025, 1, 1)) == -3 and margin(dims=(1024, 1024, 512)) == -3
    for name in ("voxel", "step"):
        for bad in (0.0, -1.0, float("nan"), float("inf")):
            assert margin(**{name: bad}) == -3, (name, bad)
    assert margin(standoff=-1e-3) == -3 and margin(standoff=float("nan")) == -3 and margin(standoff=float("inf")) == -3
    assert margin(step=2.0 ** -12, x_extent=3.0) == -3 and margin(x_extent=float("nan")) == -3
    for null in ("d", "origin3", "l", "mm", "cc"):
        assert margin(**{null: None}) == -2, null
    assert margin(B=0) == 0 and margin(B=0, d=None) == 0
    torch.cuda.synchronize()
    assert (out == float(SENTINEL)).all() and (m == SENTINEL).all() and (c == SENTINEL).all()
    assert query() == 0 and margin() == 0
    torch.cuda.synchronize()
    assert m.tolist() == [[0, 0]] * 2 and c.tolist() == [[20, 0, 36, 0]] * 2
