"""Hand paths on the device (csrc/hand_path.hip: regnet_grasp_path_check[_signed]_f32, picked by regnet_grasp_retreat_pick;
``approach.check_paths``) against tests/hand_path_reference.py, bit for bit: every output word, with sentinel rows around every
output."""
import numpy as np
import pytest
import torch

from . import approach_volume_reference as av_ref
from . import edt_reference as edt_ref
from . import hand_path_reference as ref
from . import retreat_reference as fan_ref
from .test_gpu_edt import DEV, DYADIC_BOX, IDENTITY_L, SENTINEL, TURNED, _dev

pytestmark = pytest.mark.gpu
f32 = np.float32
NONE = ref.NONE
ADIMS, AORIGIN, AVOXEL = (24, 20, 28), (-0.24, -0.20, -0.28), 0.02
RDIMS, RORIGIN, RVOXEL = (17, 9, 33), (-0.17, -0.09, -0.33), 0.02         # ragged
RBOX, RSTEP = (-0.05, 0.06, 0.01, 0.05, 0.04, -0.01), 0.01              # an 11 x 10 x 2 lattice: 2 x 2 tiles, three of them partial
TURNED_L = TURNED[:3].reshape(1, 12).astype(np.float32)
FSENT = -77.5


def _same_floats(a, b):
    """Bit for bit, but any NaN equals any NaN: the sign and payload of a NaN are not part of the contract."""
    a, b = np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32)
    nan = np.isnan(a)
    return a.shape == b.shape and np.array_equal(nan, np.isnan(b)) and np.array_equal(a[~nan].view(np.uint32), b[~nan].view(np.uint32))


def _random_field(dims, signed, seed):
    rng = np.random.default_rng(seed)
    n = dims[0] * dims[1] * dims[2]
    if not signed:
        return rng.integers(0, 500, size=n).astype(np.int32)
    words = rng.integers(1, 300, size=n)
    return np.where(rng.random(n) < 0.3, -words, words).astype(np.int32)


def _random_paths(B, R, K, seed, reach=0.3, turn=0.8):
    """(B,R,K+1,12) float32: the oblique rotation about the volume's middle, then per waypoint a growing rotation about a random
    axis and a growing shift -- poses that turn, and that leave a small volume on their way."""
    from regnet_for_3d_grasping_amd import hand_path
    rng = np.random.default_rng(seed)
    L = np.repeat(TURNED_L, B, axis=0)
    L[:, 3::4] += rng.uniform(-0.05, 0.05, size=(B, 3)).astype(np.float32)
    local = np.stack([np.concatenate([hand_path.turn_paths(rng.normal(size=(1, 3)), rng.normal(size=3), rng.uniform(-0.05, 0.05, size=3),
                                                           rng.uniform(-turn, turn) * 57.3, reach, K) for _ in range(R)])
                      for _ in range(B)])
    return ref.compose_ref(L, local)


def _check(field, dims, origin, voxel, outside, P, box, step, x_extent, thresh, signed, with_profile=True, with_disp=True,
           stream=None, compare=True):
    """The check and the pick with sentinel rows around every output -> profile, result, best, disp as numpy, each compared
    with the restatement.  ``box[1]`` may be an array: one x_hi per grasp."""
    from regnet_for_3d_grasping_amd import _lib
    P = np.ascontiguousarray(P, dtype=np.float32)
    B, R, K = P.shape[0], P.shape[1], P.shape[2] - 1
    x_lo, x_hi, ht, hw, hs, back_x = box
    per = _dev(x_hi) if np.ndim(x_hi) else None
    org = np.ascontiguousarray(np.asarray(origin, dtype=np.float32))
    Pd, fd = _dev(P), _dev(field, np.int32)
    profile = torch.full((B + 2, R, K + 1), SENTINEL, dtype=torch.int32, device=DEV)
    result = torch.full((B + 2, R, 4), SENTINEL, dtype=torch.int32, device=DEV)
    best = torch.full((B + 2, 4), SENTINEL, dtype=torch.int32, device=DEV)
    disp = torch.full((B + 2, R, K), FSENT, dtype=torch.float32, device=DEV)
    entry = "regnet_grasp_path_check_signed_f32" if signed else "regnet_grasp_path_check_f32"
    _lib.call(entry, fd, fd.data_ptr(), *dims, org.ctypes.data, float(voxel), int(outside), Pd.data_ptr(), B, R, K, float(x_lo),
              float(np.max(x_hi)) if per is not None else float(x_hi), None if per is None else per.data_ptr(), float(ht), float(hw),
              float(hs), float(back_x), float(step), float(x_extent), int(thresh), profile[1:].data_ptr() if with_profile else None,
              result[1:].data_ptr(), disp[1:].data_ptr() if with_disp else None, stream=stream)
    _lib.call("regnet_grasp_retreat_pick", result, result[1:].data_ptr(), B, R, best[1:].data_ptr(), stream=stream)
    if stream is not None:
        torch.cuda.synchronize()
    profile, result, best, disp = profile.cpu().numpy(), result.cpu().numpy(), best.cpu().numpy(), disp.cpu().numpy()
    for a in (profile, result, best):
        assert (a[[0, -1]] == SENTINEL).all()
    assert (disp[[0, -1]] == FSENT).all()
    if not with_profile:
        assert (profile == SENTINEL).all()
    if not with_disp:
        assert (disp == FSENT).all()
    profile, result, best, disp = profile[1:-1], result[1:-1], best[1:-1], disp[1:-1]
    if compare:
        want_p, want_r = ref.path_ref(field, dims, origin, voxel, outside, P, box, step, x_extent, thresh, signed)
        if with_profile:
            assert np.array_equal(profile, want_p), np.argwhere(profile != want_p)[:8]
        assert np.array_equal(result, want_r), (result, want_r)
        assert np.array_equal(best, ref.pick_ref(want_r))
        if with_disp:
            want_d = ref.disp_ref(P, box)
            assert _same_floats(disp, want_d), (disp, want_d)
    return profile, result, best, disp


@pytest.mark.parametrize("B,R,K", [(1, 1, 1), (3, 3, 2), (5, 16, 20), (1, 3, 64), (3, 1, 20), (5, 3, 1)])
def test_random_fields_and_turning_poses(B, R, K):
    """Random int32 fields, signed for odd K; both volumes (the second ragged); ``outside`` 0 and 1 with hands that leave the
    volume mid-path; a threshold in the middle of the words."""
    signed = bool(K & 1)
    for n, (dims, origin, voxel) in enumerate(((ADIMS, AORIGIN, AVOXEL), (RDIMS, RORIGIN, RVOXEL))):
        field = _random_field(dims, signed, 100 * B + 10 * R + K + n)
        P = _random_paths(B, R, K, 7 * B + R + K + n)
        for outside in (0, 1):
            profile, result, _, _ = _check(field, dims, origin, voxel, outside, P, RBOX, RSTEP, 0.06, 3, signed)
            assert (profile[:, :, 0] == profile[:, :1, 0]).all()                  # waypoint 0 is the final pose for every path
        assert (result[:, :, 3] > 0).any()                                        # some hand leaves the volume on its way


def test_hand_set_fields_empty_one_voxel_and_a_wall():
    n = ADIMS[0] * ADIMS[1] * ADIMS[2]
    P = _random_paths(3, 3, 20, 5, reach=0.08)
    empty = np.full((n,), NONE, dtype=np.int32)
    profile, result, best, _ = _check(empty, ADIMS, AORIGIN, AVOXEL, 0, P, RBOX, RSTEP, 0.06, 1, False)
    assert (profile == NONE).all() and (result[:, :, :3] == [20, NONE, NONE]).all() and (best == [0, 20, NONE, 0]).all()
    one = np.full((n,), 50, dtype=np.int32)
    inside, v = edt_ref.lookup(np.array([[0.0, 0.0, 0.0]], dtype=np.float32), P[1, 2, 7], ADIMS, AORIGIN, AVOXEL)
    assert inside.all()
    one[v[0]] = 0                                    # the voxel under the hand's origin at grasp 1, path 2, waypoint 7
    _check(one, ADIMS, AORIGIN, AVOXEL, 0, P, RBOX, RSTEP, 0.06, 1, False)
    ix = np.arange(ADIMS[0])
    wall = np.broadcast_to(np.where(ix < 6, -(6 - ix) ** 2, (ix - 5) ** 2)[None, None, :], (ADIMS[2], ADIMS[1], ADIMS[0]))
    for outside in (0, 1):
        _check(wall.reshape(-1).astype(np.int32), ADIMS, AORIGIN, AVOXEL, outside, P, RBOX, RSTEP, 0.06, 4, True)


def test_the_deciding_sample_in_every_wave_and_partial_tile_and_the_deciding_waypoint():
    """A 20 x 18 x 2 lattice: 3 x 3 tiles of 8 x 8, the last row and column partial, more tiles than the four waves.  The hand
    rises by two voxels a step, so no two of its samples ever share a voxel; one low word at a time where ONE hand sample is at
    ONE waypoint: the minimum of that waypoint comes from every wave and from the partial tiles, and from that sample alone.
    The deciding waypoint is 0 (which must not enter ``result``), 1 and K."""
    from regnet_for_3d_grasping_amd import hand_path
    box, step, x_extent = (-0.75, 0.5, 0.0625, 0.5625, 0.375, 0.0), 0.0625, 0.5
    dims, origin, voxel = (32, 20, 12), (-1.25, -0.625, -0.125), 0.0625
    assert av_ref.lattice_counts(box, 0.0, step, x_extent)[0] == (20, 18, 2)
    K = 4
    P = hand_path.straight_paths([[0, 0, 1]], K * 2 * voxel, K)[None]
    # (tile, wave): (0, 0), (0, 0), (4, 0), (1, 1), (5, 1), (2, 2), (8, 0), (7, 3), (3, 3), (6, 2); all behind the palm or in a finger
    samples = ((0, 0, 0), (7, 7, 1), (8, 8, 0), (11, 3, 1), (16, 15, 0), (19, 0, 1), (19, 17, 1), (10, 16, 0), (3, 12, 0), (1, 17, 1))
    xv, yv, zv = av_ref.lattice_samples(box, 0.0, step, x_extent)
    hand = fan_ref.hand_samples(box, step, x_extent, box[1])[3].reshape(20, 18, 2)
    for n, (i, j, k) in enumerate(samples):
        assert hand[i, j, k]
        at = (0, 1, K)[n % 3]
        point = np.array([[xv[i], yv[j], zv[k] + f32(at * 2 * voxel)]], dtype=np.float32)
        inside, v = edt_ref.lookup(point, IDENTITY_L[0], dims, origin, voxel)
        assert inside.all()
        field = np.full((dims[0] * dims[1] * dims[2],), 100, dtype=np.int32)
        field[v[0]] = 7
        profile, result, _, _ = _check(field, dims, origin, voxel, 0, P, box, step, x_extent, 50, False)
        assert profile[0, 0].tolist() == [7 if w == at else 100 for w in range(K + 1)], (i, j, k, at, profile)
        assert result[0, 0].tolist() == {0: [K, 100, 100, 0], 1: [0, NONE, 7, 0], K: [K - 1, 100, 7, 0]}[at]


def test_a_lattice_of_one_tile_leaves_three_waves_idle_and_the_threshold_boundary():
    from regnet_for_3d_grasping_amd import hand_path
    box = DYADIC_BOX                                  # 4 x 8 x 1 samples at a step of 0.25: one tile, half of it empty
    assert av_ref.lattice_counts(box, 0.0, 0.25, 0.5)[0] == (4, 8, 1)
    dims, origin = (40, 48, 4), (-4.0, -1.5, -0.25)
    ix = np.arange(dims[0])
    line = np.where(ix < 16, 0, (ix - 15) ** 2)
    field = np.broadcast_to(line[None, None, :], (dims[2], dims[1], dims[0])).reshape(-1).astype(np.int32)
    P = hand_path.straight_paths([[-1, 0, 0], [-0.5, 0.75, 0]], 3.0, 24)[None]
    profile, result, best, _ = _check(field, dims, origin, 0.125, 0, P, box, 0.25, 0.5, 1, False)
    word = int(profile[0, 0, 5])                     # exactly at the threshold the step is free, one below it it is not
    assert _check(field, dims, origin, 0.125, 0, P, box, 0.25, 0.5, word, False)[1][0, 0, :2].tolist() == [5, word]
    assert _check(field, dims, origin, 0.125, 0, P, box, 0.25, 0.5, word + 1, False)[1][0, 0, :2].tolist() == [4, int(profile[0, 0, 4])]
    for outside in (0, 1):
        _check(_random_field(dims, True, 3), dims, origin, 0.125, outside, P, box, 0.25, 0.5, 1, True)


@pytest.mark.parametrize("signed", [False, True])
def test_poses_outside_the_grid_and_a_nan_row(signed):
    field = _random_field(ADIMS, signed, 17)
    P = _random_paths(3, 2, 4, 9, reach=0.05)
    P[1, :, :, 3] += f32(5.0)                        # grasp 1: the whole hand outside the grid at every waypoint
    P[2, 1, 2, 5] = np.nan                           # a NaN row at waypoint 2 of grasp 2, path 1
    n = int(fan_ref.hand_samples(RBOX, RSTEP, 0.06, RBOX[1])[3].sum())
    for outside in (0, 1):
        profile, result, _, disp = _check(field, ADIMS, AORIGIN, AVOXEL, outside, P, RBOX, RSTEP, 0.06, 1, signed)
        edge = (-1 if signed else 0) if outside else NONE
        assert (profile[1] == edge).all() and (result[1, :, 3] == 4 * n).all()
        assert (result[1, :, 0] == (0 if outside else 4)).all()                   # skipped samples block nothing
        assert profile[2, 1, 2] == edge and result[2, 1, 3] >= n                   # no sample counted at the NaN waypoint
        assert np.isnan(disp[2, 1, 1:3]).all() and np.isfinite(disp[2, 1, [0, 3]]).all() and np.isfinite(disp[:2]).all()


def test_one_x_hi_per_grasp_null_outputs_and_two_runs():
    field = _random_field(ADIMS, True, 23)
    P = _random_paths(4, 3, 7, 2, reach=0.1)
    box = (RBOX[0], np.array([0.06, 0.03, 0.045, -0.02], dtype=np.float32)) + RBOX[2:]
    profile, result, best, disp = _check(field, ADIMS, AORIGIN, AVOXEL, 1, P, box, RSTEP, 0.06, 1, True)
    again = _check(field, ADIMS, AORIGIN, AVOXEL, 1, P, box, RSTEP, 0.06, 1, True, with_profile=False, with_disp=False)
    assert np.array_equal(again[1], result) and np.array_equal(again[2], best)             # two runs, the same bytes
    third = _check(field, ADIMS, AORIGIN, AVOXEL, 1, P, box, RSTEP, 0.06, 1, True, compare=False)
    assert np.array_equal(third[0], profile) and _same_floats(third[3], disp)
    empty = (RBOX[0], np.array([-0.06], dtype=np.float32)) + RBOX[2:]                     # x_hi below x_lo: no hand sample at all
    profile, result, _, _ = _check(field, ADIMS, AORIGIN, AVOXEL, 1, P[:1], empty, RSTEP, 0.06, 1, True)
    assert (profile == NONE).all() and result[0].tolist() == [[7, NONE, NONE, 0]] * 3


def test_translation_only_paths_give_the_retreat_fans_bytes():
    """The exact-arithmetic case of tests/test_hand_path_reference_cpu.py: ``profile`` and ``result`` of the two kernels are
    equal on the device."""
    from regnet_for_3d_grasping_amd import _lib, hand_path
    dims, origin, voxel = (40, 48, 4), (-4.0, -1.5, -0.25), 0.125
    dirs = np.array([[-1, 0, 0], [-0.5, 0.75, 0], [0.25, -1, 0.5], [0, 0, 0]], dtype=np.float32)
    K, ds = 24, 0.125
    P = hand_path.straight_paths(dirs, K * ds, K)[None]
    org = np.ascontiguousarray(np.asarray(origin, dtype=np.float32))
    x_lo, x_hi, ht, hw, hs, back_x = DYADIC_BOX
    for signed in (False, True):
        field = _random_field(dims, signed, 11)
        fd, Ld, dd = _dev(field, np.int32), _dev(IDENTITY_L), _dev(dirs)
        for outside in (0, 1):
            profile, result, _, _ = _check(field, dims, origin, voxel, outside, P, DYADIC_BOX, 0.125, 0.5, 3, signed)
            fan_p = torch.full((1, 4, K + 1), SENTINEL, dtype=torch.int32, device=DEV)
            fan_r = torch.full((1, 4, 4), SENTINEL, dtype=torch.int32, device=DEV)
            _lib.call("regnet_grasp_retreat_fan_signed_f32" if signed else "regnet_grasp_retreat_fan_f32", fd, fd.data_ptr(), *dims,
                      org.ctypes.data, voxel, outside, Ld.data_ptr(), 1, x_lo, x_hi, None, ht, hw, hs, back_x, 0.125, 0.5,
                      dd.data_ptr(), 0, 4, K, ds, 3, fan_p.data_ptr(), fan_r.data_ptr())
            assert np.array_equal(fan_p.cpu().numpy(), profile) and np.array_equal(fan_r.cpu().numpy(), result)


def test_a_side_stream_and_a_captured_graph():
    from regnet_for_3d_grasping_amd import _lib
    field = _random_field(ADIMS, True, 31)
    P = _random_paths(5, 5, 7, 4, reach=0.15)
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        _check(field, ADIMS, AORIGIN, AVOXEL, 1, P, RBOX, RSTEP, 0.06, 1, True, stream=side.cuda_stream)
    torch.cuda.synchronize()
    org = np.ascontiguousarray(np.asarray(AORIGIN, dtype=np.float32))
    fd, Pd = _dev(field, np.int32), _dev(P)
    profile = torch.full((5, 5, 8), SENTINEL, dtype=torch.int32, device=DEV)
    result = torch.full((5, 5, 4), SENTINEL, dtype=torch.int32, device=DEV)
    best = torch.full((5, 4), SENTINEL, dtype=torch.int32, device=DEV)
    disp = torch.full((5, 5, 7), FSENT, dtype=torch.float32, device=DEV)
    x_lo, x_hi, ht, hw, hs, back_x = RBOX
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        _lib.call("regnet_grasp_path_check_signed_f32", fd, fd.data_ptr(), *ADIMS, org.ctypes.data, AVOXEL, 1, Pd.data_ptr(), 5, 5, 7,
                  x_lo, x_hi, None, ht, hw, hs, back_x, RSTEP, 0.06, 1, profile.data_ptr(), result.data_ptr(), disp.data_ptr())
        _lib.call("regnet_grasp_retreat_pick", result, result.data_ptr(), 5, 5, best.data_ptr())
    other = _random_field(ADIMS, True, 37)
    fd.copy_(_dev(other, np.int32))
    graph.replay()
    torch.cuda.synchronize()
    want_p, want_r = ref.path_ref(other, ADIMS, AORIGIN, AVOXEL, 1, P, RBOX, RSTEP, 0.06, 1, True)
    assert np.array_equal(profile.cpu().numpy(), want_p) and np.array_equal(result.cpu().numpy(), want_r)
    assert np.array_equal(best.cpu().numpy(), ref.pick_ref(want_r))
    assert _same_floats(disp.cpu().numpy(), ref.disp_ref(P, RBOX))


def test_every_error_code_and_nothing_written():
    from regnet_for_3d_grasping_amd import _lib
    n = ADIMS[0] * ADIMS[1] * ADIMS[2]
    f = torch.ones((n,), dtype=torch.int32, device=DEV)
    P = _dev(np.broadcast_to(TURNED_L.reshape(1, 1, 12), (16, 65, 12)).copy())
    org = np.ascontiguousarray(np.asarray(AORIGIN, dtype=np.float32))
    out = torch.full((16 * 65 + 16 * 4,), SENTINEL, dtype=torch.int32, device=DEV)
    disp = torch.full((16 * 64,), FSENT, dtype=torch.float32, device=DEV)
    OK, SHAPE, NULL, UNSUPPORTED = 0, -1, -2, -3
    for name in ("regnet_grasp_path_check_f32", "regnet_grasp_path_check_signed_f32"):
        fn = getattr(_lib.lib, name)

        def call(dims=ADIMS, voxel=AVOXEL, outside=0, B=1, step=RSTEP, R=5, K=20, field=f.data_ptr(), origin=org.ctypes.data,
                 poses=P.data_ptr(), result=out[16 * 65:].data_ptr()):
            return fn(field, *dims, origin, voxel, outside, poses, B, R, K, *[float(v) for v in RBOX[:2]], None,
                      *[float(v) for v in RBOX[2:]], step, 0.06, 1, out.data_ptr(), result, disp.data_ptr(), None)

        for bad in (dict(B=-1), dict(outside=2), dict(outside=-1), dict(R=0), dict(K=0), dict(dims=(24, 0, 28))):
            assert call(**bad) == SHAPE, bad
        for bad in (dict(dims=(1025, 20, 28)), dict(B=1 << 31), dict(voxel=-1.0), dict(step=0.0), dict(R=17), dict(K=65),
                    dict(B=(1 << 28) // (5 * 21) + 1), dict(step=1e-7)):
            assert call(**bad) == UNSUPPORTED, bad
        for bad in (dict(field=None), dict(origin=None), dict(poses=None), dict(result=None)):
            assert call(**bad) == NULL, bad
        assert call(B=0, field=None, result=None) == OK and call(R=0, K=65, field=None) == SHAPE
        torch.cuda.synchronize()
        assert (out.cpu().numpy() == SENTINEL).all() and (disp.cpu().numpy() == FSENT).all()   # no refused call launched
        assert call(R=16, K=64) == OK
        torch.cuda.synchronize()
        got = out.cpu().numpy()
        assert (got[:16 * 65] == 1).all() and got[16 * 65:].reshape(16, 4).tolist() == [[64, 1, 1, 0]] * 16
        assert (disp.cpu().numpy() == 0.0).all()                                   # the same pose at every waypoint
        out.fill_(SENTINEL)
        disp.fill_(FSENT)


def test_check_paths_end_to_end():
    """A hand-set volume with a solid slab, three grasps: ``check_paths`` with parameters, with explicit local paths and with
    ``poses=`` as (…,12) and (…,4,4); the pick, ``waypoint`` and ``certified_steps`` equal the restatement."""
    from regnet_for_3d_grasping_amd import approach, hand_path
    from .test_gpu_edt import _hand, _volume
    dims, origin, voxel = (48, 40, 36), (-0.12, -0.10, -0.09), 0.005
    mask = np.zeros((dims[2], dims[1], dims[0]), dtype=bool)
    mask[:, 26:, :14] = True                         # a block beside and behind the hands
    vol = _volume(_hand(dims, mask.reshape(-1), origin=origin, voxel=voxel, trunc=0.01))
    field = vol.distance_field("solid", signed=True, max_distance=0.05)
    grasp = np.zeros((3, 8), dtype=np.float32)
    grasp[:, :3] = [(0.03, 0.0, 0.0), (0.035, -0.01, 0.01), (0.02, 0.012, -0.005)]
    grasp[:, 3:6] = [(0.0, 1.0, 0.0), (0.05, 1.0, 0.0), (0.0, 1.0, 0.1)]
    params = hand_path.PathParams(length=0.04, steps=8, turn_deg=25.0, pivot=(-0.02, -0.045, 0.0))
    box = av_ref.gripper_box(0.06, 0.08)
    words = field.dist2.cpu().numpy()

    def verify(check, P):
        thresh = hand_path.threshold_word(check.params.min_margin, voxel, True)
        want_p, want_r = ref.path_ref(words, dims, vol.origin, voxel, int(field.outside), P, box, voxel, 0.06, thresh, True)
        want_d = ref.disp_ref(P, box)
        best = ref.pick_ref(want_r)
        assert check.thresh == thresh and np.array_equal(check.P.cpu().numpy(), P)
        assert np.array_equal(check.profile.cpu().numpy(), want_p) and np.array_equal(check.result.cpu().numpy(), want_r)
        assert np.array_equal(check.best.cpu().numpy(), best)
        assert _same_floats(check.disp.cpu().numpy(), want_d)
        assert np.array_equal(check.waypoint.cpu().numpy(), ref.waypoint_ref(P, best))
        assert np.array_equal(check.index.cpu().numpy(), best[:, 0]) and np.array_equal(check.free_steps.cpu().numpy(), want_r[:, :, 0])
        for slack in (None, 0.0, 0.004):
            want = ref.certified_ref(want_p, want_d, voxel, True, ref.default_slack(voxel, voxel) if slack is None else slack,
                                     check.params.min_margin)
            assert np.array_equal(check.certified_steps(slack).cpu().numpy(), want), (slack, want)
        assert torch.equal(check.profile_metres, field.metres(check.profile)) and torch.equal(check.margin, field.metres(check.best[:, 2].contiguous()))
        picked = want[np.arange(3), best[:, 0]]                                   # (the last loop value: slack 0.004)
        free = ref.length_ref(want_d, best, best[:, 1])
        assert np.array_equal(check.free_length.cpu().numpy(), free)
        assert np.array_equal(check.length_at(torch.from_numpy(picked).to(DEV)).cpu().numpy(), ref.length_ref(want_d, best, picked))
        default = ref.certified_ref(want_p, want_d, voxel, True, ref.default_slack(voxel, voxel), check.params.min_margin)
        assert np.array_equal(check.certified_length.cpu().numpy(), ref.length_ref(want_d, best, default[np.arange(3), best[:, 0]]))
        for bound in (0.0, 0.011, float(free.max()), 1.0):
            assert check.passes(bound).tolist() == (free >= f32(bound)).tolist(), bound
        assert check.passes(1).tolist() == (best[:, 1] >= 1).tolist() and check.passes(int(best[:, 1].max()) + 1).tolist() == [False] * 3
        return want_r, best

    check = approach.check_paths(vol, field, _dev(grasp), 0.06, 0.08, params, to_volume=np.eye(4))
    assert isinstance(check, approach.PathCheck) and check.P.shape == (3, 9, 9, 12)
    from regnet_for_3d_grasping_amd import approach_volume
    L = approach_volume.local_to_volume(_dev(grasp), np.eye(4))[3]
    P = ref.compose_ref(L.cpu().numpy(), hand_path.default_paths(params))
    assert np.array_equal(hand_path.compose(L, hand_path.default_paths(params)).cpu().numpy(), P)      # compose, bit for bit
    result, best = verify(check, P)
    print("free steps %s, picked %s, certified %s" % (result[:, :, 0].tolist(), best[:, 0].tolist(), check.certified_steps().tolist()))
    assert (result[:, :, 0] < 8).any() and (result[:, :, 0] == 8).any()       # the block stops some paths and not others
    # explicit local paths, shared and per grasp; poses handed in directly in both layouts
    local = hand_path.default_paths(params)[[0, 5, 6]]
    verify(approach.check_paths(vol, field, _dev(grasp), 0.06, 0.08, {"paths": local, "min_margin": 0.003}), ref.compose_ref(L.cpu().numpy(), local))
    per = np.stack([local, local[::-1], local[[1, 0, 2]]])
    verify(approach.check_paths(vol, field, _dev(grasp), 0.06, 0.08, {"paths": per, "min_margin": 0.003}), ref.compose_ref(L.cpu().numpy(), per))
    direct = approach.check_paths(vol, field, _dev(grasp), 0.06, 0.08, params, poses=_dev(P))
    verify(direct, P)
    full = np.zeros(P.shape[:3] + (4, 4), dtype=np.float32)
    full[..., :3, :] = P.reshape(P.shape[:3] + (3, 4))
    full[..., 3, 3] = 1.0
    square = approach.check_paths(vol, field, _dev(grasp), 0.06, 0.08, params, poses=_dev(full))
    assert torch.equal(square.result, direct.result) and torch.equal(square.disp, direct.disp) and torch.equal(square.P, direct.P)
    with pytest.raises(ValueError, match="DistanceField of this volume"):
        approach.check_paths(vol, None, _dev(grasp), 0.06, 0.08, params)
    with pytest.raises(ValueError, match="signed field"):
        approach.check_paths(vol, vol.distance_field("solid"), _dev(grasp), 0.06, 0.08, {"min_margin": -0.001})
    with pytest.raises(ValueError, match="poses must be"):
        approach.check_paths(vol, field, _dev(grasp), 0.06, 0.08, params, poses=_dev(P[:2]))
