"""The retreat fan on the device (csrc/retreat.hip: regnet_grasp_retreat_fan[_signed]_f32, regnet_grasp_retreat_pick;
``approach.retreat_fan``) against tests/retreat_reference.py, bit for bit: every output word, with sentinel words around every
output."""
import numpy as np
import pytest
import torch

from . import approach_volume_reference as av_ref
from . import edt_reference as edt_ref
from . import retreat_reference as ref
from .test_gpu_edt import DEV, DYADIC_BOX, IDENTITY_L, MDIMS, MORIGIN, SENTINEL, TURNED, _dev, _hand, _volume

pytestmark = pytest.mark.gpu
f32 = np.float32
NONE = ref.NONE
RDIMS, RORIGIN, RVOXEL = (37, 29, 23), (-0.30, -0.25, -0.20), 0.02       # ragged dims: 0.74 x 0.58 x 0.46 m about the origin
RBOX, RSTEP = (-0.05, 0.06, 0.01, 0.05, 0.04, -0.01), 0.01              # an 11 x 10 x 2 lattice: 2 x 2 tiles, three of them partial
WDIMS, WORIGIN, WVOXEL = (40, 48, 4), (-4.0, -1.5, -0.25), 0.125          # the wall scene of tests/test_retreat_reference_cpu.py
TURNED_L = TURNED[:3].reshape(1, 12).astype(np.float32)


def _random_field(dims, signed, seed):
    rng = np.random.default_rng(seed)
    n = dims[0] * dims[1] * dims[2]
    if not signed:
        return rng.integers(0, 500, size=n).astype(np.int32)
    words = rng.integers(1, 300, size=n)
    return np.where(rng.random(n) < 0.3, -words, words).astype(np.int32)


def _fan(field, dims, origin, voxel, outside, L, box, step, x_extent, dirs, K, ds, thresh, signed, with_profile=True, stream=None,
         check=True):
    """The two entry points with sentinel rows around every output -> profile, result, best as numpy, each compared with the
    restatement.  ``box[1]`` may be an array: one x_hi per grasp."""
    from regnet_for_3d_grasping_amd import _lib
    L = np.ascontiguousarray(L, dtype=np.float32).reshape(-1, 12)
    B = L.shape[0]
    dirs = np.ascontiguousarray(dirs, dtype=np.float32)
    R = dirs.shape[-2]
    x_lo, x_hi, ht, hw, hs, back_x = box
    per = _dev(x_hi) if np.ndim(x_hi) else None
    org = np.ascontiguousarray(np.asarray(origin, dtype=np.float32))
    Ld, dd, fd = _dev(L), _dev(dirs), _dev(field, np.int32)
    profile = torch.full((B + 2, R, K + 1), SENTINEL, dtype=torch.int32, device=DEV)
    result = torch.full((B + 2, R, 4), SENTINEL, dtype=torch.int32, device=DEV)
    best = torch.full((B + 2, 4), SENTINEL, dtype=torch.int32, device=DEV)
    entry = "regnet_grasp_retreat_fan_signed_f32" if signed else "regnet_grasp_retreat_fan_f32"
    _lib.call(entry, fd, fd.data_ptr(), *dims, org.ctypes.data, float(voxel), int(outside), Ld.data_ptr(), B, float(x_lo),
              float(np.max(x_hi)) if per is not None else float(x_hi), None if per is None else per.data_ptr(), float(ht), float(hw),
              float(hs), float(back_x), float(step), float(x_extent), dd.data_ptr(), 3 * R if dirs.ndim == 3 else 0, R, K, float(ds),
              int(thresh), profile[1:].data_ptr() if with_profile else None, result[1:].data_ptr(), stream=stream)
    _lib.call("regnet_grasp_retreat_pick", result, result[1:].data_ptr(), B, R, best[1:].data_ptr(), stream=stream)
    if stream is not None:
        torch.cuda.synchronize()
    profile, result, best = profile.cpu().numpy(), result.cpu().numpy(), best.cpu().numpy()
    for a in (profile, result, best):
        assert (a[[0, -1]] == SENTINEL).all()
    if not with_profile:
        assert (profile == SENTINEL).all()
    profile, result, best = profile[1:-1], result[1:-1], best[1:-1]
    if check:
        want_p, want_r = ref.fan_ref(field, dims, origin, voxel, outside, L, box, step, x_extent, dirs, K, ds, thresh, signed)
        if with_profile:
            assert np.array_equal(profile, want_p), np.argwhere(profile != want_p)[:8]
        assert np.array_equal(result, want_r), (result, want_r)
        assert np.array_equal(best, ref.pick_ref(want_r))
    return profile, result, best


def _grasp_rows(B, seed):
    """B local-to-volume rows: the oblique rotation shifted about the volume, the last one far enough to leave it on its way."""
    rng = np.random.default_rng(seed)
    L = np.repeat(TURNED_L, B, axis=0)
    L[:, 3::4] += rng.uniform(-0.08, 0.08, size=(B, 3)).astype(np.float32)
    L[-1, 3] += f32(0.22)
    return L


@pytest.mark.parametrize("B", [1, 5])
@pytest.mark.parametrize("R", [1, 5, 16])
@pytest.mark.parametrize("K", [1, 7, 64])
def test_random_fields_of_ragged_dims(B, R, K):
    """Random int32 fields, signed for odd R; ``outside`` 0 and 1 with hands that leave the volume mid-path, along directions that are not unit vectors; one shared table of
    directions for B = 1 and per-grasp tables for B = 5; a threshold in the middle of the words."""
    signed = bool(R & 1)
    field = _random_field(RDIMS, signed, 100 * B + 10 * R + K)
    rng = np.random.default_rng(K + R)
    dirs = rng.normal(size=((B, R, 3) if B > 1 else (R, 3)))
    dirs = (dirs / np.linalg.norm(dirs, axis=-1, keepdims=True) * rng.uniform(1.0, 1.5, size=dirs.shape[:-1] + (1,))).astype(np.float32)
    L = _grasp_rows(B, R)
    hands = int(ref.hand_samples(RBOX, RSTEP, 0.06, RBOX[1])[3].sum())
    ds = 0.8 / K                                     # a path of 0.8 m or more: longer than the volume's half diagonal, 0.52 m
    for outside in (0, 1):
        profile, result, _ = _fan(field, RDIMS, RORIGIN, RVOXEL, outside, L, RBOX, RSTEP, 0.06, dirs, K, ds, 3, signed)
        assert (result[:, :, 3] > 0).all()                                    # every hand leaves the volume on its way, mid-path
        assert (result[:, :, 3] < K * hands).all() or K == 1
        assert (profile[:, :, 0] == profile[:, :1, 0]).all()                  # step 0 is the final pose for every direction


def _planted(lattice_box, step, x_extent, dims, origin, voxel, samples, shift):
    """For each lattice sample (i, j, k): a field of 100s with one 7, in the voxel the sample reaches after ``shift`` steps of one
    voxel along -x -> (field, the sample) pairs."""
    xv, yv, zv = av_ref.lattice_samples(lattice_box, 0.0, step, x_extent)
    out = []
    for i, j, k in samples:
        point = np.array([[xv[i] - f32(shift * voxel), yv[j], zv[k]]], dtype=np.float32)
        inside, v = edt_ref.lookup(point, IDENTITY_L[0], dims, origin, voxel)
        assert inside.all()
        field = np.full((dims[0] * dims[1] * dims[2],), 100, dtype=np.int32)
        field[v[0]] = 7
        out.append((field, (i, j, k)))
    return out


def test_the_deciding_sample_in_every_wave_and_in_the_partial_tiles():
    """A 20 x 18 x 2 lattice: 3 x 3 tiles of 8 x 8, the last row and column partial, more tiles than the four waves.  One low word
    at a time where a different hand sample arrives after three steps of one voxel: the minimum of step 3 comes from every wave
    and from the partial tiles, and from that sample alone."""
    box, step, x_extent = (-0.75, 0.5, 0.0625, 0.5625, 0.375, 0.0), 0.0625, 0.5
    dims, origin, voxel = (32, 20, 4), (-1.25, -0.625, -0.125), 0.0625
    assert av_ref.lattice_counts(box, 0.0, step, x_extent)[0] == (20, 18, 2)
    dirs = np.array([[-1, 0, 0]], dtype=np.float32)
    # (tile, wave): (0, 0), (0, 0), (4, 0), (1, 1), (5, 1), (2, 2), (8, 0), (7, 3), (3, 3), (6, 2); all behind the palm or in a finger
    samples = ((0, 0, 0), (7, 7, 1), (8, 8, 0), (11, 3, 1), (16, 15, 0), (19, 0, 1), (19, 17, 1), (10, 16, 0), (3, 12, 0), (1, 17, 1))
    _, _, _, hand = ref.hand_samples(box, step, x_extent, box[1])
    hand = hand.reshape(20, 18, 2)
    for field, (i, j, k) in _planted(box, step, x_extent, dims, origin, voxel, samples, 3):
        assert hand[i, j, k], (i, j, k)
        profile, result, _ = _fan(field, dims, origin, voxel, 0, IDENTITY_L, box, step, x_extent, dirs, 4, voxel, 50, False)
        assert profile[0, 0, 3] == 7 and result[0, 0, 2] == 7, (i, j, k, profile)


def test_a_lattice_of_one_tile_leaves_three_waves_idle():
    box = DYADIC_BOX                                  # 4 x 8 x 1 samples at a step of 0.25: one tile, half of it empty
    assert av_ref.lattice_counts(box, 0.0, 0.25, 0.5)[0] == (4, 8, 1)
    field = _random_field(MDIMS, True, 3)
    dirs = np.array([[-1, 0, 0], [-0.5, 0.5, 0], [0, -1, 0]], dtype=np.float32)
    for outside in (0, 1):
        _fan(field, MDIMS, MORIGIN, 0.25, outside, IDENTITY_L, box, 0.25, 0.5, dirs, 6, 0.25, 1, True)


def _wall_field(wall=16, behind=None):
    ix = np.arange(WDIMS[0])
    line = np.where(ix < wall, 0, (ix - (wall - 1)) ** 2)
    field = np.broadcast_to(line[None, None, :], (WDIMS[2], WDIMS[1], WDIMS[0])).copy()
    if behind is not None:
        field[:, :, :behind] = 9
    return field.reshape(-1).astype(np.int32)


def _wall(field, thresh, K=24, ds=0.125, dirs=((-1, 0, 0),)):
    return _fan(field, WDIMS, WORIGIN, WVOXEL, 0, IDENTITY_L, DYADIC_BOX, 0.125, 0.5, np.asarray(dirs, dtype=np.float32), K, ds, thresh,
                False)


def test_the_threshold_exactly_and_one_below_and_where_a_path_is_blocked():
    """The hand of the dyadic box backs into the wall of the CPU tests: the rearmost samples' word falls step by step,
    (13 - k)^2 for k <= 12 and 0 from step 13 on."""
    field = _wall_field()
    profile, result, _ = _wall(field, 1)
    assert profile[0, 0].tolist() == [(13 - k) ** 2 if k <= 12 else 0 for k in range(25)]
    assert result[0, 0].tolist() == [12, 1, 0, 0]
    word = int(profile[0, 0, 5])                     # exactly at the threshold the step is free, one below it it is not
    assert _wall(field, word)[1][0, 0].tolist() == [5, word, 0, 0]
    assert _wall(field, word + 1)[1][0, 0].tolist() == [4, int(profile[0, 0, 4]), 0, 0]
    assert _wall(field, 145)[1][0, 0].tolist() == [0, NONE, 0, 0]                       # blocked at k = 1 (144 < 145)
    assert _wall(field, 1, K=13)[1][0, 0].tolist() == [12, 1, 0, 0]                      # blocked only at k = K
    assert _wall(field, 1, K=12)[1][0, 0].tolist() == [12, 1, 1, 0]                      # free throughout
    assert _wall(field, 0)[1][0, 0].tolist() == [24, 0, 0, 0]                            # (word 0 passes a threshold of 0)
    # free space again behind a wall four voxels thick: a later free step after a blocked one does not extend the prefix
    profile, result, _ = _wall(_wall_field(behind=12), 1)
    assert profile[0, 0, 13] == 0 and profile[0, 0, 24] == 9 and result[0, 0].tolist() == [12, 1, 0, 0]
    # ... and tilted away by 60 degrees the whole path is free, so the pick prefers it
    tilted = ((-1, 0, 0), (-0.5, np.sqrt(0.75), 0))
    _, result, best = _wall(field, 1, dirs=tilted)
    assert result[0, 0, 0] == 12 and result[0, 1, 0] >= 21 and best[0, 0] == 1


def test_every_branch_of_the_picks_tie_rule():
    from regnet_for_3d_grasping_amd import _lib
    rows = [[[3, 5], [4, 1], [4, 2], [4, 2], [0, NONE]],                  # more steps; then the larger margin; then the smaller r
            [[0, NONE], [0, NONE], [0, NONE], [0, NONE], [0, NONE]],       # all equal: the first
            [[2, 9], [2, 9], [2, 10], [1, 50], [2, 10]],                   # a larger margin does not beat more steps
            [[1, -4], [1, -9], [1, -4], [0, NONE], [1, -5]],               # signed margins
            [[5, 1], [5, 1], [5, 1], [5, 1], [6, -7]]]                     # the last direction wins on steps alone
    want = [[2, 4, 2, 0], [0, 0, NONE, 0], [2, 2, 10, 0], [0, 1, -4, 0], [4, 6, -7, 0]]
    B = 300                                          # more than one workgroup of lanes
    table = np.zeros((B, 5, 4), dtype=np.int32)
    table[:, :, 2:] = 12345                          # columns 2 and 3 are not read
    for b in range(B):
        table[b, :, :2] = rows[b % 5]
    result = _dev(table, np.int32)
    best = torch.full((B + 2, 4), SENTINEL, dtype=torch.int32, device=DEV)
    _lib.call("regnet_grasp_retreat_pick", result, result.data_ptr(), B, 5, best[1:].data_ptr())
    best = best.cpu().numpy()
    assert (best[[0, -1]] == SENTINEL).all()
    assert np.array_equal(best[1:-1], ref.pick_ref(table)) and best[1:6].tolist() == want
    one = torch.full((3, 4), SENTINEL, dtype=torch.int32, device=DEV)      # R = 1
    _lib.call("regnet_grasp_retreat_pick", result, result.data_ptr(), 1, 1, one[1:].data_ptr())
    assert one.cpu().numpy().tolist() == [[SENTINEL] * 4, [0, 3, 5, 0], [SENTINEL] * 4]


@pytest.mark.parametrize("signed", [False, True])
def test_outside_samples_nan_rows_and_nan_directions(signed):
    field = _random_field(RDIMS, signed, 17)
    L = np.repeat(TURNED_L, 3, axis=0)
    L[1, 5] = np.nan                                 # a NaN row: every lookup of the grasp is OUTSIDE
    dirs = np.array([[-1, 0, 0], [np.nan, 0, 0], [0, 0, np.inf], [-100, 0, 0]], dtype=np.float32)
    _, _, _, hand = ref.hand_samples(RBOX, RSTEP, 0.06, RBOX[1])
    n = int(hand.sum())
    for outside in (0, 1):
        profile, result, _ = _fan(field, RDIMS, RORIGIN, RVOXEL, outside, L, RBOX, RSTEP, 0.06, dirs, 4, 0.01, 1, signed)
        edge = (-1 if signed else 0) if outside else NONE
        assert (profile[1] == edge).all() and (result[1, :, 3] == 4 * n).all()
        # a NaN or infinite direction: 0 * NaN is a NaN, so step 0 is OUTSIDE too, but only steps 1..K are counted
        assert (profile[0, 1:3] == edge).all() and (result[0, 1:3, 3] == 4 * n).all()
        # a metre a step along -x leaves the volume at once: step 0 is inside, the others are not
        assert profile[0, 3, 0] == profile[0, 0, 0] and (profile[0, 3, 1:] == edge).all() and result[0, 3, 3] == 4 * n
        assert result[0, 0, 3] == 0
        # skipped samples block nothing; counted ones read -1, or the unsigned 0, below the threshold of 1
        assert result[1, 0, 0] == (0 if outside else 4) and result[0, 3, 0] == (0 if outside else 4)


def test_one_x_hi_per_grasp_and_no_profile():
    field = _random_field(RDIMS, True, 23)
    L = _grasp_rows(4, 2)
    box = (RBOX[0], np.array([0.06, 0.03, 0.045, -0.02], dtype=np.float32)) + RBOX[2:]
    dirs = np.array([[-1, 0, 0], [-0.8, 0.6, 0]], dtype=np.float32)
    counts = [int(ref.hand_samples(box, RSTEP, 0.06, xh)[3].sum()) for xh in box[1]]
    assert counts[0] > counts[2] > counts[1] > counts[3] > 0
    profile, result, best = _fan(field, RDIMS, RORIGIN, RVOXEL, 1, L, box, RSTEP, 0.06, dirs, 7, 0.02, 1, True)
    again = _fan(field, RDIMS, RORIGIN, RVOXEL, 1, L, box, RSTEP, 0.06, dirs, 7, 0.02, 1, True, with_profile=False)
    assert np.array_equal(again[1], result) and np.array_equal(again[2], best)             # two runs, the same bytes
    empty = (RBOX[0], np.array([-0.06], dtype=np.float32)) + RBOX[2:]                     # x_hi below x_lo: no hand sample at all
    profile, result, _ = _fan(field, RDIMS, RORIGIN, RVOXEL, 1, TURNED_L, empty, RSTEP, 0.06, dirs, 7, 0.02, 1, True)
    assert (profile == NONE).all() and result[0].tolist() == [[7, NONE, NONE, 0]] * 2


def test_a_side_stream_and_a_captured_graph():
    from regnet_for_3d_grasping_amd import _lib
    field = _random_field(RDIMS, True, 31)
    L = _grasp_rows(5, 4)
    dirs = np.random.default_rng(2).normal(size=(5, 3)).astype(np.float32)
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        _fan(field, RDIMS, RORIGIN, RVOXEL, 1, L, RBOX, RSTEP, 0.06, dirs, 7, 0.03, 1, True, stream=side.cuda_stream)
    torch.cuda.synchronize()
    org = np.ascontiguousarray(np.asarray(RORIGIN, dtype=np.float32))
    fd, Ld, dd = _dev(field, np.int32), _dev(L), _dev(dirs)
    profile = torch.full((5, 5, 8), SENTINEL, dtype=torch.int32, device=DEV)
    result = torch.full((5, 5, 4), SENTINEL, dtype=torch.int32, device=DEV)
    best = torch.full((5, 4), SENTINEL, dtype=torch.int32, device=DEV)
    x_lo, x_hi, ht, hw, hs, back_x = RBOX
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        _lib.call("regnet_grasp_retreat_fan_signed_f32", fd, fd.data_ptr(), *RDIMS, org.ctypes.data, RVOXEL, 1, Ld.data_ptr(), 5,
                  x_lo, x_hi, None, ht, hw, hs, back_x, RSTEP, 0.06, dd.data_ptr(), 0, 5, 7, 0.03, 1, profile.data_ptr(),
                  result.data_ptr())
        _lib.call("regnet_grasp_retreat_pick", result, result.data_ptr(), 5, 5, best.data_ptr())
    other = _random_field(RDIMS, True, 37)
    fd.copy_(_dev(other, np.int32))
    graph.replay()
    torch.cuda.synchronize()
    want_p, want_r = ref.fan_ref(other, RDIMS, RORIGIN, RVOXEL, 1, L, RBOX, RSTEP, 0.06, dirs, 7, 0.03, 1, True)
    assert np.array_equal(profile.cpu().numpy(), want_p) and np.array_equal(result.cpu().numpy(), want_r)
    assert np.array_equal(best.cpu().numpy(), ref.pick_ref(want_r))


def test_every_error_code_and_nothing_written():
    from regnet_for_3d_grasping_amd import _lib
    n = RDIMS[0] * RDIMS[1] * RDIMS[2]
    f = torch.ones((n,), dtype=torch.int32, device=DEV)
    L, d = _dev(TURNED_L), _dev(np.array([[-1, 0, 0]] * 16, dtype=np.float32))
    org = np.ascontiguousarray(np.asarray(RORIGIN, dtype=np.float32))
    out = torch.full((16 * 65 + 16 * 4,), SENTINEL, dtype=torch.int32, device=DEV)
    OK, SHAPE, NULL, UNSUPPORTED = 0, -1, -2, -3
    for name in ("regnet_grasp_retreat_fan_f32", "regnet_grasp_retreat_fan_signed_f32"):
        fn = getattr(_lib.lib, name)

        def call(dims=RDIMS, voxel=RVOXEL, outside=0, B=1, step=RSTEP, stride=0, R=5, K=20, ds=0.005, field=f.data_ptr(),
                 origin=org.ctypes.data, rows=L.data_ptr(), dirs=d.data_ptr(), result=out[16 * 65:].data_ptr()):
            return fn(field, *dims, origin, voxel, outside, rows, B, *[float(v) for v in RBOX[:2]], None,
                      *[float(v) for v in RBOX[2:]], step, 0.06, dirs, stride, R, K, ds, 1, out.data_ptr(), result, None)

        for bad in (dict(B=-1), dict(outside=2), dict(outside=-1), dict(R=0), dict(K=0), dict(stride=-1), dict(dims=(37, 0, 23))):
            assert call(**bad) == SHAPE, bad
        for bad in (dict(dims=(1025, 29, 23)), dict(B=1 << 31), dict(voxel=-1.0), dict(step=0.0), dict(R=17), dict(K=65),
                    dict(B=(1 << 28) // (5 * 21) + 1), dict(ds=-1e-3), dict(ds=float("nan")), dict(ds=float("inf")), dict(step=1e-7)):
            assert call(**bad) == UNSUPPORTED, bad
        for bad in (dict(field=None), dict(origin=None), dict(rows=None), dict(dirs=None), dict(result=None)):
            assert call(**bad) == NULL, bad
        assert call(B=0, field=None, result=None) == OK and call(R=0, K=65, field=None) == SHAPE
        torch.cuda.synchronize()
        assert (out.cpu().numpy() == SENTINEL).all()                                      # no refused call launched
        assert call(ds=0.0) == OK and call(R=16, K=64, ds=0.001) == OK
        torch.cuda.synchronize()
        got = out.cpu().numpy()
        assert (got[:16 * 65] == 1).all() and got[16 * 65:].reshape(16, 4).tolist() == [[64, 1, 1, 0]] * 16
        out.fill_(SENTINEL)
    pick = _lib.lib.regnet_grasp_retreat_pick
    assert pick(out.data_ptr(), -1, 5, out.data_ptr(), None) == SHAPE and pick(out.data_ptr(), 1, 0, out.data_ptr(), None) == SHAPE
    assert pick(out.data_ptr(), 1, 17, out.data_ptr(), None) == UNSUPPORTED
    assert pick(None, 1, 5, out.data_ptr(), None) == NULL and pick(out.data_ptr(), 1, 5, None, None) == NULL
    assert pick(None, 0, 5, None, None) == OK


def test_retreat_fan_tilts_away_from_a_wall_planted_over_a_rendered_box():
    """Two rendered views of a box on a table, integrated on the device; a grasp over the box approaches straight down.  A solid
    slab planted 3 cm above the hand's back, over the half space x < 0, blocks the straight retreat and the fan's other three
    directions; the one tilted towards +x slides out from under it: it is free over its whole length and the pick takes it."""
    from regnet_for_3d_grasping_amd import approach, retreat, tsdf
    from .icp_projective_reference import look_at, rectangle, render
    W, H, K = 128, 96, (120.0, 120.0, 63.5, 47.5)
    x, y, t = 0.03, 0.03, 0.06
    scene = [rectangle((-0.5, -0.5, 0.0), (1.0, 0, 0), (0, 1.0, 0)), rectangle((-x, -y, t), (2 * x, 0, 0), (0, 2 * y, 0)),
             rectangle((-x, -y, 0.0), (2 * x, 0, 0), (0, 0, t)), rectangle((-x, y, 0.0), (2 * x, 0, 0), (0, 0, t)),
             rectangle((-x, -y, 0.0), (0, 2 * y, 0), (0, 0, t)), rectangle((x, -y, 0.0), (0, 2 * y, 0), (0, 0, t))]
    dims = (48, 40, 60)
    vol = tsdf.Volume(tsdf.TsdfParams(voxel=0.005, trunc=0.01, origin=(-0.12, -0.10, -0.015), dims=dims, max_points=1 << 13), DEV)
    for eye in ((0.0, -0.35, 0.30), (0.0, 0.35, 0.30)):
        pose = look_at(eye, (0.0, 0.0, 0.03))
        vol.integrate((_dev(render(scene, W, H, K, pose)), None, W, H, K), pose)
    nx, ny, nz = dims
    vol.D.view(nz, ny, nx)[37:41, :, :24] = -0.5     # z in [0.17, 0.19), x < 0: the hand's back ends at z = 0.14
    vol.W.view(nz, ny, nx)[37:41, :, :24] = 1
    field = vol.distance_field("solid", signed=True, max_distance=0.05)
    grasp = np.zeros((2, 8), dtype=np.float32)
    grasp[:, :3] = [(0.0, 0.0, 0.08), (0.004, 0.003, 0.085)]
    grasp[:, 3:6] = [(0.0, 1.0, 0.0), (0.05, 1.0, 0.0)]
    grasp[:, 6] = -np.pi / 2                         # approach straight down
    params = retreat.RetreatParams(length=0.08, steps=16, tilt_deg=35.0)
    fan = approach.retreat_fan(vol, field, _dev(grasp), 0.06, 0.08, params, to_volume=np.eye(4))
    assert isinstance(fan, approach.RetreatFan) and fan.thresh == 1 and fan.dirs.shape == (5, 3)
    box = av_ref.gripper_box(0.06, 0.08)
    want_p, want_r = ref.fan_ref(field.dist2.cpu().numpy(), dims, vol.origin, 0.005, 0, fan.L.cpu().numpy(), box, 0.005, 0.06,
                                 fan.dirs.cpu().numpy(), 16, 0.08 / 16, 1, True)
    assert np.array_equal(fan.profile.cpu().numpy(), want_p) and np.array_equal(fan.result.cpu().numpy(), want_r)
    assert np.array_equal(fan.best.cpu().numpy(), ref.pick_ref(want_r))
    steps = fan.free_steps.cpu().numpy()
    index = fan.index.cpu().numpy()
    direction = fan.direction.cpu().numpy()
    print("free steps %s, picked %s, direction %s, margin %s" % (steps.tolist(), index.tolist(), direction.tolist(),
                                                                 fan.margin.tolist()))
    assert (steps[:, 0] < 10).all() and (steps[:, 0] >= 4).all()              # straight: 3 cm of 5 mm steps, give or take the lattice
    assert (index != 0).all() and (steps[np.arange(2), index] == 16).all()
    assert (np.delete(steps, index[0], axis=1) < 16).all()                    # the other four directions run into the slab
    assert (direction[:, 0] > 0.5).all() and (direction[:, 2] > 0.7).all()    # tilted towards +x, and up
    assert np.allclose(np.linalg.norm(direction, axis=1), 1.0, atol=1e-5)
    assert torch.equal(fan.free_length, torch.full((2,), 16, device=DEV) * float(f32(0.08 / 16)))
    assert torch.equal(fan.pregrasp, fan.center + fan.direction * fan.free_length.unsqueeze(1))
    assert torch.equal(fan.profile_metres, field.metres(fan.profile)) and torch.equal(fan.margin, field.metres(fan.best[:, 2].contiguous()))
    assert (fan.margin > 0).all()
    # the threshold at its boundary word on the device's own conversion
    for bound in (0.0, 0.004, float(fan.margin[0])):
        word = retreat.threshold_word(bound, 0.005, True)
        below = -1 if word == 1 else word - 1
        got = field.metres(torch.tensor([below, word], dtype=torch.int32, device=DEV)).cpu().numpy()
        assert got[0] < f32(bound) <= got[1], (bound, word, got)
    with pytest.raises(ValueError, match="DistanceField of this volume"):
        approach.retreat_fan(vol, None, _dev(grasp), 0.06, 0.08, params)
    small = _volume(_hand(MDIMS))
    with pytest.raises(ValueError, match="DistanceField of this volume"):
        approach.retreat_fan(vol, small.distance_field("solid"), _dev(grasp), 0.06, 0.08, params)
    with pytest.raises(ValueError, match="signed field"):
        approach.retreat_fan(vol, vol.distance_field("solid"), _dev(grasp), 0.06, 0.08, {"min_margin": -0.001})
    # analyse_volume carries the fan when its parameters ask for one
    res = approach.analyse_volume(vol, _dev(grasp), 0.06, 0.08, dict(space="volume", field=True, field_signed=True, retreat=params,
                                                                     min_retreat=0.08), to_volume=np.eye(4), field=field)
    assert torch.equal(res.retreat.best, fan.best) and res.passes().tolist() == [True, True]
    # a third hand whose back lies INSIDE the slab has no free step in any direction, and min_retreat drops it alone
    three = np.concatenate([grasp, grasp[:1]])
    three[2, :3] = (-0.05, 0.0, 0.12)
    res = approach.analyse_volume(vol, _dev(three), 0.06, 0.08, dict(space="volume", field=True, field_signed=True, retreat=params,
                                                                     min_retreat=0.01), to_volume=np.eye(4), field=field)
    assert res.retreat.free_steps.cpu().numpy()[2].tolist() == [0] * 5 and res.passes().tolist() == [True, True, False]
    assert float(res.retreat.free_length[2]) == 0.0 and float(res.retreat.margin[2]) == float("inf")
    assert torch.equal(res.retreat.pregrasp[2], res.retreat.center[2])
    up = approach.retreat_fan(vol, field, _dev(grasp), 0.06, 0.08, retreat.RetreatParams(length=0.08, steps=16, up=(1.0, 0.0, 1.0)))
    assert up.dirs.shape == (2, 7, 3) and np.allclose(up.dirs.norm(dim=2).cpu().numpy(), 1.0, atol=1e-5)
    lifted = (up.frame.to(torch.float32) @ up.dirs[:, 5].unsqueeze(2)).squeeze(2).cpu().numpy()
    assert np.allclose(lifted, np.array([1.0, 0.0, 1.0]) / np.sqrt(2.0), atol=1e-5)
