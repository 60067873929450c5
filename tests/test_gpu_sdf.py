"""The signed, capped distance field of the TSDF volume on the MI355X (csrc/edt.hip: regnet_tsdf_sdf, the signed metres, the
interpolating query and the signed margin, and through tsdf.Volume.distance_field / DistanceField.query /
approach.analyse_volume) against the all-pairs numpy restatement (tests/sdf_reference.py).  Every comparison is bit for bit.
Volumes are set by hand through ``Volume.D`` / ``Volume.W`` (the helpers of tests/test_gpu_edt.py)."""
import numpy as np
import pytest
import torch

from . import edt_reference as edt_ref
from . import sdf_reference as ref
from .test_gpu_edt import (DEV, DYADIC_BOX, GUARD, IDENTITY_L, MDIMS, MORIGIN, SENTINEL, TURNED, _at, _dev, _hand, _mask, _mv,
                           _random_mask, _volume)

pytestmark = pytest.mark.gpu
f32 = np.float32
NONE = ref.NONE


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _sdf(vol, mode=0, outside=0, sign=1, cap=0, nearest=True, margin=0.0, min_weight=None, stream=None):
    """regnet_tsdf_sdf on a ``tsdf.Volume`` -> (field, nearest or None) as numpy arrays; the outputs and the workspace sit in the
    middle of guarded buffers whose sentinel words must survive."""
    from regnet_for_3d_grasping_amd import _lib
    p = vol.params
    n = p.dims[0] * p.dims[1] * p.dims[2]
    size = int(_lib.lib.regnet_tsdf_sdf_workspace_bytes(*p.dims, int(sign), int(nearest)))
    assert size == (n * 4 * (2 if nearest else 1) if sign else 0)
    planes = [torch.full((n + 2 * GUARD,), SENTINEL, dtype=torch.int32, device=DEV) for _ in range(2 if nearest else 1)]
    work = torch.full((size // 4 + 2 * GUARD,), SENTINEL, dtype=torch.int32, device=DEV)
    _lib.call("regnet_tsdf_sdf", vol.data, vol.data.data_ptr(), *p.dims, float(p.trunc),
              int(p.min_weight if min_weight is None else min_weight), float(margin), int(mode), int(outside), int(sign), int(cap),
              planes[0][GUARD:].data_ptr(), planes[1][GUARD:].data_ptr() if nearest else None,
              work[GUARD:].data_ptr() if size else None, stream=stream)
    out = [t.cpu().numpy() for t in planes + [work]]
    for a in out:
        assert (a[:GUARD] == SENTINEL).all() and (a[-GUARD:] == SENTINEL).all()
    return out[0][GUARD:-GUARD], (out[1][GUARD:-GUARD] if nearest else None)


def _check(dims, mask, caps=(0, 1, 2, 7), what=""):
    """Device against restatement on the volume whose SOLID voxels are ``mask``: both signs, outside 0 / 1, every cap, with
    ``nearest``; without it the field alone, signed, at the first and the last cap."""
    mask = np.asarray(mask, dtype=bool)
    vol = _volume(_hand(dims, mask))
    for outside in (0, 1):
        signed = ref.transform(mask, dims, bool(outside), 1, 0)
        # (sign 0 is the positive part, 0 / the voxel itself on an obstacle: tests/test_sdf_reference_cpu.py holds that relation)
        unsigned = (np.where(mask, 0, signed[0]), np.where(mask, np.arange(len(mask)), signed[1]))
        for sign in (0, 1):
            base = signed if sign else unsigned
            for cap in caps:
                want = ref.apply_cap(base[0], base[1], cap)
                got = _sdf(vol, 0, outside, sign, cap)
                where = (what, dims, outside, sign, cap)
                assert got[0].dtype == np.int32 and got[1].dtype == np.int32
                assert np.array_equal(got[0], want[0]), (where, np.flatnonzero(got[0] != want[0])[:8])
                assert np.array_equal(got[1], want[1]), (where, np.flatnonzero(got[1] != want[1])[:8])
                if sign:
                    assert (got[0] != 0).all()
                if sign and cap in (caps[0], caps[-1]):
                    alone = _sdf(vol, 0, outside, sign, cap, nearest=False)
                    assert alone[1] is None and np.array_equal(alone[0], want[0]), where


DIMS = [(5, 3, 2), (33, 17, 9), (70, 1, 1), (1, 1, 64), (1024, 2, 1), (65, 3, 2)]


@pytest.mark.parametrize("dims", DIMS, ids=lambda d: "%dx%dx%d" % d)
def test_field_on_masks(dims):
    n = dims[0] * dims[1] * dims[2]
    largest = int(np.sqrt(sum((d - 1) ** 2 for d in dims)))
    caps = (0, 1, 2, 7, min(max(largest, 1), 1023))
    _check(dims, np.zeros((n,), dtype=bool), caps, "empty")
    _check(dims, np.ones((n,), dtype=bool), caps, "full")
    single = (dims[0] // 2, dims[1] // 2, dims[2] // 2)
    _check(dims, _mask(dims, [single]), caps, "single")
    _check(dims, ~_mask(dims, [single]), caps, "single free voxel")
    _check(dims, _mask(dims, [(0, 0, 0)]), caps, "corner")
    _check(dims, _random_mask(dims, 0.05), caps, "random 5%")
    _check(dims, _random_mask(dims, 0.6, seed=1), caps, "random 60%")


def test_the_cap_equal_to_the_largest_distance_changes_nothing_and_a_distance_of_exactly_the_cap_keeps_its_nearest():
    dims = (12, 9, 1)
    mask = _mask(dims, [(0, 0, 0)])
    vol = _volume(_hand(dims, mask))
    field, near = _sdf(vol, cap=5)
    want = ref.transform(mask, dims, cap=5)
    assert np.array_equal(field, want[0]) and np.array_equal(near, want[1])
    assert field[_at(dims, 5, 0, 0)] == 25 and near[_at(dims, 5, 0, 0)] == 0
    assert field[_at(dims, 3, 4, 0)] == 25 and near[_at(dims, 3, 4, 0)] == 0        # 9 + 16: exactly the cap
    assert field[_at(dims, 4, 4, 0)] == 25 and near[_at(dims, 4, 4, 0)] == -1       # 32: saturated
    # the largest distance is sqrt(11^2 + 8^2) = 13.6: a cap of 14 changes nothing
    capped, uncapped = _sdf(vol, cap=14), _sdf(vol, cap=0)
    assert np.array_equal(capped[0], uncapped[0]) and np.array_equal(capped[1], uncapped[1])
    # the negative side: a solid block with one free voxel, exactly 5 away along y
    dims = (3, 9, 2)
    free = _mask(dims, [(1, 1, 0)])
    field, near = _sdf(_volume(_hand(dims, ~free)), cap=5)
    want = ref.transform(~free, dims, cap=5)
    assert np.array_equal(field, want[0]) and np.array_equal(near, want[1])
    assert field[_at(dims, 1, 6, 0)] == -25 and near[_at(dims, 1, 6, 0)] == _at(dims, 1, 1, 0)
    assert field[_at(dims, 1, 7, 0)] == -25 and near[_at(dims, 1, 7, 0)] == -1


def test_ties_across_a_tile_boundary_on_both_sides():
    """The y / z passes stage ``regnet_edt_tile`` consecutive ix per workgroup: ties whose two candidates lie in different tiles,
    as obstacles (the positive side) and as the only free voxels of a solid block (the negative side); 0 + 25 = 9 + 16 too."""
    from regnet_for_3d_grasping_amd import _lib
    dims = (70, 9, 7)
    tiles = {int(_lib.lib.regnet_edt_tile(n, 1)) for n in dims[1:]}
    assert tiles == {64}
    pair = _mask(dims, [(61, 4, 3), (67, 4, 3), (64, 0, 3), (64, 8, 3)])     # (64, 4, 3): 9 = 9 across the boundary, 16 = 16 along y
    also = _mask(dims, [(5, 0, 0), (3, 4, 0)])                              # (0, 0, 0): 25 = 9 + 16
    for mask in (pair | also, ~(pair | also)):
        vol = _volume(_hand(dims, mask))
        for cap in (0, 5):
            got, want = _sdf(vol, cap=cap), ref.transform(mask, dims, cap=cap)
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
        centre = _at(dims, 64, 4, 3)
        assert abs(int(got[0][centre])) == 9 and got[1][centre] == _at(dims, 61, 4, 3)
        assert abs(int(got[0][0])) == 25 and got[1][0] == _at(dims, 5, 0, 0)


@pytest.mark.parametrize("mode", [0, 1])
def test_classification_at_the_thresholds_and_nan_distances(mode):
    dims = (9, 5, 3)
    n = 9 * 5 * 3
    rng = np.random.default_rng(17)
    hand = _hand(dims, None, trunc=0.5, min_weight=3)
    d_solid = f32(0.125 / 0.5)
    hand.D[:] = rng.choice(np.array([d_solid, np.nextafter(d_solid, f32(-1)), np.nextafter(d_solid, f32(1)), -1.0, 1.0, np.nan],
                                    dtype=np.float32), n)
    hand.W[:] = rng.choice(np.array([0, 2, 3, 4], dtype=np.int32), n)
    vol = _volume(hand)
    for outside in (0, 1):
        for cap in (0, 2):
            got = _sdf(vol, mode, outside, 1, cap, margin=0.125)
            want = ref.sdf_ref(hand.D, hand.W, dims, 0.5, 3, 0.125, mode, bool(outside), 1, cap)
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    assert (got[0] < 0).any() and (got[0] > 0).any()


def test_sign_0_cap_0_is_the_unsigned_entry_byte_for_byte_and_two_runs_agree():
    from .test_gpu_edt import _kernel
    dims = (67, 33, 5)
    vol = _volume(_hand(dims, _random_mask(dims, 0.02)))
    for outside in (0, 1):
        for nearest in (True, False):
            old = _kernel(vol, 0, outside, nearest)
            new = _sdf(vol, 0, outside, 0, 0, nearest)
            assert old[0].tobytes() == new[0].tobytes()
            assert (old[1] is None and new[1] is None) or old[1].tobytes() == new[1].tobytes()
    a, b = _sdf(vol, 0, 1, 1, 7), _sdf(vol, 0, 1, 1, 7)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()


def test_a_side_stream_and_a_captured_graph():
    dims = (33, 17, 9)
    mask = _random_mask(dims, 0.3)
    vol = _volume(_hand(dims, mask))
    want = ref.transform(mask, dims, True, 1, 3)
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        got = _sdf(vol, 0, 1, 1, 3, stream=side.cuda_stream)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    field = vol.distance_field("solid", outside=True, nearest=True, signed=True, max_distance=3 * vol.params.voxel)
    assert field.signed and field.cap == 3 and field.work is not None
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        vol.distance_field("solid", outside=True, nearest=True, signed=True, max_distance=3 * vol.params.voxel, out=field)
    other = _random_mask(dims, 0.3, seed=5)
    vol.D.copy_(_dev(_hand(dims, other).D))
    graph.replay()
    torch.cuda.synchronize()
    want = ref.transform(other, dims, True, 1, 3)
    assert np.array_equal(field.dist2.cpu().numpy(), want[0]) and np.array_equal(field.nearest.cpu().numpy(), want[1])


def test_field_error_codes():
    from regnet_for_3d_grasping_amd import _lib
    vol = _volume(_hand((6, 8, 2)))
    f = torch.zeros((96,), dtype=torch.int32, device=DEV)
    w = torch.zeros((192,), dtype=torch.int32, device=DEV)

    def call(volume=vol.data.data_ptr(), dims=(6, 8, 2), trunc=1.0, min_weight=1, margin=0.0, mode=0, outside=0, sign=1, cap=0,
             field=f.data_ptr(), nearest=None, work=w.data_ptr()):
        return _lib.lib.regnet_tsdf_sdf(volume, dims[0], dims[1], dims[2], trunc, min_weight, margin, mode, outside, sign, cap,
                                        field, nearest, work, None)

    OK, SHAPE, UNSUPPORTED, NULL = 0, -1, _lib.lib.regnet_edt_tile(0, 0), call(volume=None)
    assert call() == OK and call(sign=0, work=None) == OK and call(cap=1023) == OK
    assert NULL not in (OK, SHAPE, UNSUPPORTED) and UNSUPPORTED not in (OK, SHAPE)
    for bad in (dict(sign=2), dict(sign=-1), dict(cap=-1), dict(mode=2), dict(outside=-1), dict(min_weight=0), dict(dims=(0, 8, 2))):
        assert call(**bad) == SHAPE, bad
    for bad in (dict(cap=1024), dict(dims=(1025, 1, 1)), dict(min_weight=1 << 31), dict(trunc=float("nan")), dict(margin=1e300)):
        assert call(**bad) == UNSUPPORTED, bad
    assert call(field=None) == NULL and call(work=None) == NULL
    assert call(sign=2, cap=2000, field=None) == SHAPE                     # the first rule broken
    assert _lib.lib.regnet_tsdf_sdf_workspace_bytes(6, 8, 2, 0, 1) == 0
    assert _lib.lib.regnet_tsdf_sdf_workspace_bytes(6, 8, 2, 1, 0) == 384
    assert _lib.lib.regnet_tsdf_sdf_workspace_bytes(6, 8, 2, 1, 1) == 768
    assert (f.cpu().numpy() != 0).all()                                    # (only the successful calls wrote)


# ---- the signed metres and the query -------------------------------------------------------------------------------------------
QDIMS, QORIGIN, QVOXEL = (9, 7, 5), (-0.031, 0.017, 0.4), 0.005


def _query(field, nearest, dims, origin, voxel, points, T12, interpolate, gradient=True, stride=None):
    from regnet_for_3d_grasping_amd import _lib
    f, nr = _dev(field, np.int32), _dev(nearest, np.int32)
    pts = _dev(points)
    if stride is not None:                                                  # the points as columns of a wider, transposed buffer
        wide = torch.full((5, pts.shape[0] * 2), 7.0, dtype=torch.float32, device=DEV)
        wide[1:4, ::2] = pts.t()
        pts = wide[1:4, ::2].t()
        assert pts.stride() == (2, wide.shape[1])
    M = int(pts.shape[0])
    origin = np.ascontiguousarray(np.asarray(origin, dtype=np.float32))
    rows = np.ascontiguousarray(np.asarray(T12, dtype=np.float32).reshape(12))
    dist = torch.full((M + 2,), -7.0, dtype=torch.float32, device=DEV)
    grad = torch.full((M + 2, 3), -7.0, dtype=torch.float32, device=DEV)
    xyz = torch.full((M + 2, 3), -7.0, dtype=torch.float32, device=DEV)
    _lib.call("regnet_edt_query_signed_f32", f, f.data_ptr(), None if nr is None else nr.data_ptr(), *dims, origin.ctypes.data,
              float(voxel), pts.data_ptr(), pts.stride(0), pts.stride(1), M, rows.ctypes.data, int(interpolate), dist[1:].data_ptr(),
              grad[1:].data_ptr() if gradient else None, xyz[1:].data_ptr())
    dist, grad, xyz = dist.cpu().numpy(), grad.cpu().numpy(), xyz.cpu().numpy()
    assert dist[0] == -7 and dist[-1] == -7 and (grad[[0, -1]] == -7).all() and (xyz[[0, -1]] == -7).all()
    if not gradient:
        assert (grad == -7).all()
    return dist[1:-1], grad[1:-1], xyz[1:-1]


def _query_points(dims, origin, voxel):
    """Voxel centres, points on faces and one ulp either side, points in the rim and outside, NaN rows, random points."""
    o = np.asarray(origin, dtype=np.float32)
    v = f32(voxel)
    rng = np.random.default_rng(23)
    centres = (o[None, :] + (edt_ref.coords(dims).astype(np.float32) + f32(0.5)) * v).astype(np.float32)
    faces = (o[None, :] + rng.integers(0, np.array(dims) + 1, (60, 3)).astype(np.float32) * v).astype(np.float32)
    span = (np.array(dims, dtype=np.float64) + 1.0) * float(v)
    anywhere = (o.astype(np.float64) - 0.5 * float(v) + rng.random((300, 3)) * span).astype(np.float32)   # the rim and beyond
    rim = anywhere.copy()
    rim[:, 0] = o[0] + f32(0.2) * v
    bad = np.array([[np.nan, 0.42, 0.41], [0.0, np.inf, 0.41], [-0.02, 0.03, -np.inf]], dtype=np.float32)
    return np.concatenate([centres, faces, np.nextafter(faces, f32(np.inf)), np.nextafter(faces, f32(-np.inf)), anywhere, rim, bad])


@pytest.mark.parametrize("cap", [0, 3])
def test_query_distance_gradient_and_nearest(cap):
    dims, origin, voxel = QDIMS, QORIGIN, QVOXEL
    mask = _random_mask(dims, 0.3, seed=2)
    field, nearest = ref.transform(mask, dims, False, 1, cap)
    points = _query_points(dims, origin, voxel)
    identity = np.eye(4, dtype=np.float32)[:3].reshape(12)
    for interpolate in (0, 1):
        want = ref.query_signed_ref(field, nearest, dims, origin, voxel, points, identity, bool(interpolate))
        for gradient in (True, False):
            got = _query(field, nearest, dims, origin, voxel, points, identity, interpolate, gradient)
            assert np.array_equal(_bits(got[0]), _bits(want[0])), np.flatnonzero(_bits(got[0]) != _bits(want[0]))[:8]
            assert np.array_equal(_bits(got[2]), _bits(want[2]))
            if gradient:
                assert np.array_equal(_bits(got[1]), _bits(want[1])), np.flatnonzero((_bits(got[1]) != _bits(want[1])).any(axis=1))[:8]
    n = dims[0] * dims[1] * dims[2]
    plain = _query(field, nearest, dims, origin, voxel, points, identity, 0)
    assert np.array_equal(_bits(plain[0][:n]), _bits(ref.metres_signed_ref(field, voxel)))      # a centre: the voxel's own value
    assert (_bits(plain[1]) == 0x7fc00000).all()                                                # no interpolation: no gradient
    if cap:                                          # on a dyadic lattice t is exactly 0 at a centre: the corner value comes back
        centres = (np.array([-1.0, -1.0, -0.5], dtype=np.float32)[None, :] + (edt_ref.coords(dims).astype(np.float32) + f32(0.5)) * f32(0.25))
        exact = _query(field, nearest, dims, (-1.0, -1.0, -0.5), 0.25, centres, identity, 1)
        assert np.array_equal(_bits(exact[0]), _bits(ref.metres_signed_ref(field, 0.25)))
    assert np.isnan(got[0][-3:]).all() and (_bits(got[0][-3:]) == 0x7fc00000).all()
    # strided points through a to_volume
    inverse = np.linalg.inv(TURNED)
    local = (np.concatenate([points[:400], np.ones((400, 1))], axis=1) @ inverse.T)[:, :3].astype(np.float32)
    rows = TURNED[:3].astype(np.float32).reshape(12)
    want = ref.query_signed_ref(field, nearest, dims, origin, voxel, local, rows, True)
    got = _query(field, nearest, dims, origin, voxel, local, rows, 1, True, stride=True)
    for g, w in zip(got, want):
        assert np.array_equal(_bits(g), _bits(w))


def test_query_with_none_corners_and_the_python_interface():
    dims, origin, voxel = QDIMS, QORIGIN, QVOXEL
    points = _query_points(dims, origin, voxel)
    identity = np.eye(4, dtype=np.float32)[:3].reshape(12)
    n = dims[0] * dims[1] * dims[2]
    for mask in (np.zeros((n,), dtype=bool), np.ones((n,), dtype=bool)):       # every corner +NONE / -NONE: +-inf, inf - inf = NaN
        field, nearest = ref.transform(mask, dims)
        want = ref.query_signed_ref(field, nearest, dims, origin, voxel, points, identity, True)
        got = _query(field, nearest, dims, origin, voxel, points, identity, 1)
        for g, w in zip(got, want):
            assert np.array_equal(_bits(g), _bits(w))
        assert (_bits(got[0])[np.isnan(got[0])] == 0x7fc00000).all() and (_bits(got[1])[np.isnan(got[1])] == 0x7fc00000).all()
    mask = _random_mask(dims, 0.3, seed=2)
    vol = _volume(_hand(dims, mask, origin, voxel))
    sdf = vol.distance_field("solid", nearest=True, signed=True, max_distance=0.0149)          # 2.98 voxels: a cap of 3
    assert sdf.signed and sdf.cap == 3
    field, nearest = ref.transform(mask, dims, False, 1, 3)
    assert np.array_equal(sdf.dist2.cpu().numpy(), field) and np.array_equal(sdf.nearest.cpu().numpy(), nearest)
    assert np.array_equal(_bits(sdf.metres().cpu().numpy()), _bits(ref.metres_signed_ref(field, voxel)))
    want = ref.query_signed_ref(field, nearest, dims, origin, voxel, points, identity, True)
    d, g, xyz = sdf.query(_dev(points), nearest=True, interpolate=True, gradient=True)
    for got, w in zip((d, g, xyz), want):
        assert np.array_equal(_bits(got.cpu().numpy()), _bits(w))
    plain = ref.query_signed_ref(field, nearest, dims, origin, voxel, points, identity, False)
    assert np.array_equal(_bits(sdf.query(_dev(points)).cpu().numpy()), _bits(plain[0]))
    turned = sdf.query(_dev(points), to_volume=TURNED, interpolate=True, gradient=True, gradient_frame="points")[1]
    in_volume = sdf.query(_dev(points), to_volume=TURNED, interpolate=True, gradient=True)[1]
    ok = torch.isfinite(in_volume).all(dim=1)
    assert torch.allclose(turned[ok], in_volume[ok] @ torch.from_numpy(TURNED[:3, :3].astype(np.float32)).to(DEV), atol=1e-5)
    unsigned = vol.distance_field("solid", max_distance=0.0149)                                 # capped and unsigned
    assert not unsigned.signed and unsigned.cap == 3 and unsigned.work is None
    assert np.array_equal(unsigned.dist2.cpu().numpy(), ref.transform(mask, dims, False, 0, 3)[0])
    with pytest.raises(ValueError):
        unsigned.query(_dev(points), interpolate=True)
    with pytest.raises(ValueError):
        sdf.query(_dev(points), gradient=True)
    with pytest.raises(ValueError):
        vol.distance_field("solid", max_distance=-1.0)
    with pytest.raises(ValueError):
        vol.distance_field("solid", signed=True, out=unsigned)
    again = vol.distance_field("solid", nearest=True, signed=True, out=sdf)
    assert again is sdf and sdf.cap == 0 and np.array_equal(sdf.dist2.cpu().numpy(), ref.transform(mask, dims)[0])


def test_query_and_metres_error_codes():
    from regnet_for_3d_grasping_amd import _lib
    f = torch.ones((12,), dtype=torch.int32, device=DEV)
    pts = torch.zeros((4, 3), dtype=torch.float32, device=DEV)
    out = torch.zeros((4,), dtype=torch.float32, device=DEV)
    origin, rows = np.zeros(3, dtype=np.float32), np.eye(4, dtype=np.float32)[:3].reshape(12).copy()

    def call(field=f.data_ptr(), dims=(3, 2, 2), voxel=0.5, points=pts.data_ptr(), M=4, interpolate=1, distance=out.data_ptr()):
        return _lib.lib.regnet_edt_query_signed_f32(field, None, dims[0], dims[1], dims[2], origin.ctypes.data, voxel, points, 3, 1, M,
                                                    rows.ctypes.data, interpolate, distance, None, None, None)

    OK, SHAPE, UNSUPPORTED, NULL = 0, -1, _lib.lib.regnet_edt_tile(0, 0), call(field=None)
    assert call() == OK and call(M=0, field=None) == OK
    assert call(M=-1) == SHAPE and call(interpolate=2) == SHAPE and call(dims=(0, 2, 2)) == SHAPE
    assert call(dims=(1025, 1, 1)) == UNSUPPORTED and call(voxel=0.0) == UNSUPPORTED and call(M=1 << 31) == UNSUPPORTED
    assert call(points=None) == NULL and call(distance=None) == NULL
    m = _lib.lib.regnet_edt_metres_signed_f32
    assert m(f.data_ptr(), 4, 0.5, out.data_ptr(), None) == OK and m(None, 0, 0.5, None, None) == OK
    assert m(f.data_ptr(), -1, 0.5, out.data_ptr(), None) == SHAPE and m(f.data_ptr(), 4, -0.5, out.data_ptr(), None) == UNSUPPORTED
    assert m(None, 4, 0.5, out.data_ptr(), None) == NULL and m(f.data_ptr(), 4, 0.5, None, None) == NULL


# ---- the signed margin -----------------------------------------------------------------------------------------------------------
def _margin(field, dims, origin, voxel, outside, L, box, standoff, step, x_extent):
    from regnet_for_3d_grasping_amd import _lib
    L = _dev(L)
    B = int(L.shape[0])
    x_lo, x_hi, ht, hw, hs, back_x = box
    origin = np.ascontiguousarray(np.asarray(origin, dtype=np.float32))
    margins = torch.full((B + 2, 2), SENTINEL, dtype=torch.int32, device=DEV)
    counts = torch.full((B + 2, 6), SENTINEL, dtype=torch.int32, device=DEV)
    f = _dev(field, np.int32)
    _lib.call("regnet_grasp_margin_volume_signed_f32", f, f.data_ptr(), *dims, origin.ctypes.data, float(voxel), int(outside),
              L.data_ptr(), B, float(x_lo), float(x_hi), None, float(ht), float(hw), float(hs), float(back_x), float(standoff),
              float(step), float(x_extent), margins[1:].data_ptr(), counts[1:].data_ptr())
    margins, counts = margins.cpu().numpy(), counts.cpu().numpy()
    assert (margins[[0, -1]] == SENTINEL).all() and (counts[[0, -1]] == SENTINEL).all()
    got = margins[1:-1], counts[1:-1]
    want = ref.margin_signed_ref(field, dims, origin, voxel, outside, L.cpu().numpy(), box, standoff, step, x_extent)
    assert np.array_equal(got[0], want[0]), (got[0], want[0])
    assert np.array_equal(got[1], want[1]), (got[1], want[1])
    return got


def _dyadic(obstacles, outside=0, L=IDENTITY_L):
    mask = _mask(MDIMS, obstacles)
    field, _ = _sdf(_volume(_hand(MDIMS, mask, MORIGIN, 0.25)), 0, outside, 1, 0)
    assert np.array_equal(field, ref.transform(mask, MDIMS, bool(outside))[0])
    margins, counts = _margin(field, MDIMS, MORIGIN, 0.25, outside, L, DYADIC_BOX, 0.5, 0.25, 0.5)
    return margins[0].tolist(), counts[0].tolist()


def test_signed_margin_rules_on_hand_set_volumes():
    # the lattice of tests/test_gpu_edt.py: 20 hand samples, 36 swept samples, all voxel centres of the 12 x 12 x 1 volume
    assert _dyadic([]) == ([NONE, NONE], [20, 0, 36, 0, 0, 0])                                    # free
    assert _dyadic([_mv(0.875, 0.875)]) == ([4, 4], [20, 0, 36, 0, 0, 0])                         # free, two voxels beyond a tip
    assert _dyadic([_mv(-0.375, 0.375)]) == ([-1, -1], [20, 0, 36, 0, 1, 1])                      # grazing: one hand sample in a voxel
    assert _dyadic([_mv(-0.875, 0.125)]) == ([4, -1], [20, 0, 36, 0, 0, 1])                       # a blocker's voxel, two from the back
    # inside a block: every voxel with x < 0.5 is solid; the deepest hand sample is the back's at x = -0.375, 4 voxels from
    # the free voxels at x > 0.5; the deepest swept sample the blocker at x = -0.875, 6 voxels
    block = [(ix, iy, 0) for ix in range(8) for iy in range(12)]
    margins, counts = _dyadic(block)
    assert margins == [-16, -36] and counts == [20, 0, 36, 0, 20, 36]


def test_signed_margin_outside_samples_nan_rows_and_no_grasp():
    L = IDENTITY_L.copy()
    L[0, 3] = 1.25                                   # the far lane leaves the volume: 2 hand samples OUTSIDE
    for outside in (0, 1):
        margins, counts = _dyadic([_mv(-1.375, -1.375)], outside, L)
        assert counts == [20, 2, 36, 2, 2 * outside, 2 * outside]
        assert margins == ([-1, -1] if outside else [85, 53])
    bad = np.repeat(IDENTITY_L, 3, axis=0)
    bad[1, 5] = np.nan
    field = ref.transform(_mask(MDIMS, [_mv(0.875, 0.875)]), MDIMS)[0]
    for outside in (0, 1):
        margins, counts = _margin(field, MDIMS, MORIGIN, 0.25, outside, bad, DYADIC_BOX, 0.5, 0.25, 0.5)
        assert counts[1].tolist() == [20, 20, 36, 36, 20 * outside, 36 * outside]
        assert margins[1].tolist() == ([-1, -1] if outside else [NONE, NONE])
        assert margins[0].tolist() == [4, 4] and margins[2].tolist() == [4, 4]
    margins, counts = _margin(field, MDIMS, MORIGIN, 0.25, 0, np.zeros((0, 12), dtype=np.float32), DYADIC_BOX, 0.5, 0.25, 0.5)
    assert margins.shape == (0, 2) and counts.shape == (0, 6)


def test_the_deciding_sample_in_every_wave_and_in_the_partial_tiles():
    """A 20 x 16 x 2 lattice: 3 x 2 tiles of 8 x 8, the last column of tiles partial, more tiles than the four waves.  One solid
    voxel at a time under a different swept sample, so that the minimum comes from every wave and from the partial tiles."""
    from . import approach_volume_reference as av_ref
    box, standoff, step, x_extent = (-0.5, 0.5, 0.0625, 0.5, 0.375, 0.0), 0.25, 0.0625, 0.5
    dims, origin, voxel = (24, 16, 4), (-0.875, -0.5, -0.125), 0.0625
    (n_x, n_y, n_z), _, _ = av_ref.lattice_counts(box, standoff, step, x_extent)
    assert (n_x, n_y, n_z) == (20, 16, 2)
    xv, yv, zv = av_ref.lattice_samples(box, standoff, step, x_extent)
    # (tile, wave) = (0, 0), (0, 0), (4, 0), (1, 1), (5, 1), (2, 2), (5, 1), (4, 0), (3, 3)
    for i, j, k in ((0, 0, 0), (7, 7, 1), (8, 8, 0), (11, 3, 1), (16, 15, 0), (19, 0, 1), (19, 15, 1), (10, 9, 0), (3, 12, 0)):
        inside, v = edt_ref.lookup(np.array([[xv[i], yv[j], zv[k]]], dtype=np.float32), IDENTITY_L[0], dims, origin, voxel)
        assert inside.all()
        mask = np.zeros((24 * 16 * 4,), dtype=bool)
        mask[v[0]] = True
        field = ref.transform(mask, dims)[0]
        margins, counts = _margin(field, dims, origin, voxel, 0, IDENTITY_L, box, standoff, step, x_extent)
        assert margins[0, 1] == -1 and counts[0, 5] == 1, (i, j, k, margins, counts)


def test_analyse_volume_reads_a_signed_field():
    """Every voxel with x < 0.5 of the 12 x 12 x 1 volume is solid and the hand sits at the origin, sampled every centimetre: all
    its samples lie within 0.16 m of the origin, in the voxel columns ix = 5 (x < 0, three voxels from the free column 8) and
    ix = 6 (two voxels), and the hand has samples on both sides of x = 0 whichever way it is turned."""
    from regnet_for_3d_grasping_amd import approach
    block = [(ix, iy, 0) for ix in range(8) for iy in range(12)]
    vol = _volume(_hand(MDIMS, _mask(MDIMS, block), MORIGIN, 0.25))
    sdf = vol.distance_field("solid", signed=True)
    grasp = torch.tensor([[0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0]], dtype=torch.float32, device=DEV)
    params = dict(space="volume", field=True, field_signed=True, min_margin=0.0, step=0.01)
    res = approach.analyse_volume(vol, grasp, 0.06, 0.08, params, field=sdf)
    assert res.margin_counts.shape == (1, 6)
    counts = res.margin_counts.cpu().numpy()[0]
    assert counts[0] > 0 and counts[2] > counts[0] and counts[1] == 0 and counts[3] == 0
    assert res.margins.cpu().numpy().tolist() == [[-9, -9]]
    assert int(res.colliding_hand[0]) == counts[0] == counts[4] and int(res.colliding_sweep[0]) == counts[2] == counts[5]
    want = sdf.metres(res.margins.t().contiguous())
    assert torch.equal(res.margin_hand, want[0]) and torch.equal(res.margin_sweep, want[1])
    assert float(res.margin_hand[0]) == -0.625 and float(res.margin_sweep[0]) == -0.625       # -(3 - 0.5) voxels of 0.25 m
    assert not bool(res.passes()[0])
    tolerant = approach.analyse_volume(vol, grasp, 0.06, 0.08, dict(params, min_margin=-0.625), field=sdf)
    assert bool(tolerant.passes()[0])                                                           # a tolerated penetration
    assert not bool(approach.analyse_volume(vol, grasp, 0.06, 0.08, dict(params, min_margin=-0.5), field=sdf).passes()[0])
    assert sdf.bytes() == 2 * 4 * 144 and vol.distance_field("solid", nearest=True, signed=True).bytes() == 4 * 4 * 144
    unsigned = approach.analyse_volume(vol, grasp, 0.06, 0.08, dict(space="volume", field=True, step=0.01),
                                       field=vol.distance_field("solid"))
    assert unsigned.margin_counts.shape == (1, 4) and unsigned.colliding_hand is None
    assert unsigned.margins.cpu().numpy().tolist() == [[0, 0]]
    with pytest.raises(ValueError):
        approach.ApproachParams(space="volume", field_signed=True)
    with pytest.raises(ValueError):
        approach.ApproachParams(space="volume", field=True, min_margin=-0.001)                 # negative only on a signed field
