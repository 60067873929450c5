"""The three grasp entry points agree about one hand (csrc/hand_box.h holds their one definition of its sets): on the same cloud,
grasps and box the collision scan, the antipodal statistics and the approach analysis give the same integers and the same bits.
Each side is also held against the numpy restatement (tests/approach_reference.py), so a shared mistake is no agreement.

The box is the dyadic one of ``approach_reference.known_cases()`` and every coordinate a multiple of 1/16, so that all local
coordinates are exact in float32: a point put on a face IS on the face, and with strict comparisons it is outside."""
import functools

import numpy as np
import pytest
import torch

from . import approach_reference as ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
X_LO, X_HI, HT, HW, HS, BACK_X = ref.DYADIC_BOX
STANDOFF, CONTACT_DEPTH, COS_FRICTION = ref.DYADIC["standoff"], ref.DYADIC["contact_depth"], ref.DYADIC["cos_friction"]
PER_GRASP_X_HI = np.array([0.5, 0.125, 0.25], dtype=np.float32)
SIZES = (0, 1, 63, 257)      # no point, one lane, a partial wave, one point beyond the 256-thread stride
nan = float("nan")

GRASPS = np.array([
    np.eye(4),
    [[0, 1, 0, 0], [-1, 0, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1]],                       # a quarter turn: x = py, y = -px
    [[1, 0, 0, -0.25], [0, 1, 0, 0.125], [0, 0, 1, 0], [0, 0, 0, 1]],                # a translation
], dtype=np.float32)

SPECIAL = [
    [0.25, 0.5, 0.0],                                          # between the fingers (the one point of N = 1)
    [-0.25, 0.0, 0.0],                                         # behind the palm
    [0.25, 0.875, 0.0], [0.25, -0.875, 0.0],                   # inside either finger
    [-1.0, 0.0, 0.0], [-1.0, 0.875, 0.0],                      # the sweep corridor: inner and finger lane
    [X_LO, 0.0, 0.0], [X_HI, 0.0, 0.0], [BACK_X, 0.0, 0.0],    # on the faces across x, the palm's among them
    [X_LO - STANDOFF, 0.0, 0.0],                               # on the far end of the sweep
    [0.25, HS, 0.0], [0.25, -HS, 0.0],                         # on the fingers' inner faces: neither region nor finger
    [0.25, HW, 0.0], [0.25, -HW, 0.0],                         # on their outer faces
    [0.25, 0.0, HT], [0.25, 0.0, -HT], [0.25, 0.875, HT],      # on the faces across z
    [-0.25, HW, 0.0], [-1.0, 0.0, -HT],                        # behind the palm and in the corridor, on a face
    [nan, 0.0, 0.0], [0.25, nan, 0.0], [0.25, 0.5, nan],       # a NaN coordinate: in no set
]


@functools.lru_cache(maxsize=None)
def _cloud():
    """257 rows: the special points, then a fixed draw of multiples of 1/16 in [-2, 2]^2 x [-1/4, 1/4]; unit normals along axes."""
    rng = np.random.RandomState(11)
    n_fill = SIZES[-1] - len(SPECIAL)
    fill = np.stack((rng.randint(-32, 33, n_fill), rng.randint(-32, 33, n_fill), rng.randint(-4, 5, n_fill)), 1) / 16.0
    points = np.concatenate((np.asarray(SPECIAL), fill)).astype(np.float32)
    normals = np.eye(3, dtype=np.float32)[rng.randint(0, 3, len(points))] * rng.choice([-1.0, 0.5], (len(points), 1)).astype(np.float32)
    points.setflags(write=False)
    normals.setflags(write=False)
    return points, normals


def _dev(a, strided):
    """``a`` (N,3) on the device; ``strided``: as a view of every other row and column of a larger tensor."""
    t = torch.from_numpy(np.array(a, dtype=np.float32)).to(DEV)      # (a copy: the shared cloud is read-only)
    if not strided:
        return t
    wide = torch.full((2 * t.shape[0], 6), 99.0, dtype=torch.float32, device=DEV)
    wide[::2, ::2] = t
    view = wide[::2, ::2]
    assert not view.is_contiguous() or t.shape[0] == 0
    return view


def _run(N, per_grasp, strided):
    """-> collision counts (B,4), antipodal stats (B,4), approach counts (B,8) and values (B,4), and the restatement's pair."""
    from regnet_for_3d_grasping_amd import _lib
    points, normals = (a[:N] for a in _cloud())
    p, n, T = _dev(points, strided), _dev(normals, strided), torch.from_numpy(GRASPS).to(DEV)
    B = T.shape[0]
    per = torch.from_numpy(PER_GRASP_X_HI).to(DEV) if per_grasp else None
    box = (X_LO, 0.0 if per_grasp else X_HI, per.data_ptr() if per_grasp else None, HT, HW, HS, BACK_X)
    coll = torch.full((B, 4), -77, dtype=torch.int32, device=DEV)
    stats = torch.full((B, 4), -77.0, dtype=torch.float32, device=DEV)
    sides = torch.full((B, 2), -77, dtype=torch.int32, device=DEV)
    counts = torch.full((B, 8), -77, dtype=torch.int32, device=DEV)
    values = torch.full((B, 4), -77.0, dtype=torch.float32, device=DEV)
    cloud = (p.data_ptr(), p.stride(0), p.stride(1))
    with_normals = cloud + (n.data_ptr(), n.stride(0), n.stride(1))
    _lib.call("regnet_grasp_collision_counts_f32", p, *cloud, N, T.data_ptr(), B, *box, coll.data_ptr())
    _lib.call("regnet_grasp_antipodal_stats_f32", p, *with_normals, N, T.data_ptr(), B, *box, CONTACT_DEPTH, stats.data_ptr(),
              sides.data_ptr())
    _lib.call("regnet_grasp_approach_f32", p, *with_normals, N, T.data_ptr(), B, *box, STANDOFF, CONTACT_DEPTH, COS_FRICTION,
              counts.data_ptr(), values.data_ptr())
    ref_box = (X_LO, PER_GRASP_X_HI if per_grasp else X_HI, HT, HW, HS, BACK_X)
    want = ref.approach_ref(points, normals, GRASPS, ref_box, STANDOFF, CONTACT_DEPTH, COS_FRICTION)
    return coll.cpu().numpy(), stats.cpu().numpy(), counts.cpu().numpy(), values.cpu().numpy(), want


@pytest.mark.parametrize("per_grasp", [False, True], ids=["scalar_depth", "x_hi_per_grasp"])
@pytest.mark.parametrize("N", SIZES)
def test_kernels_agree_about_the_hand(N, per_grasp):
    coll, stats, counts, values, want = _run(N, per_grasp, strided=False)
    # the kernels among themselves
    assert np.array_equal(coll[:, 3], counts[:, 0]), (coll, counts)                    # the region
    assert np.array_equal(coll[:, 1] + coll[:, 2], counts[:, 2]), (coll, counts)       # back + finger: the hand
    full = counts[:, 0] > 0
    assert stats[full, 1].tobytes() == values[full, 0].tobytes(), (stats, values)      # y_min
    assert stats[full, 0].tobytes() == values[full, 1].tobytes(), (stats, values)      # y_max
    # ... and each against the restatement
    assert np.array_equal(counts, want[0]), (counts, want[0])
    assert values.tobytes() == want[1].tobytes(), (values, want[1])
    assert np.array_equal(coll[:, 3], want[0][:, 0]) and np.array_equal(coll[:, 1] + coll[:, 2], want[0][:, 2]), (coll, want[0])
    assert stats[full, 1].tobytes() == want[1][full, 0].tobytes() and stats[full, 0].tobytes() == want[1][full, 1].tobytes()
    if N >= 63:                                      # the cloud holds every special point: the sets are not vacuously equal
        assert full[0] and counts[0, 2] > 0 and counts[0, 1] > 0, counts
    if N == 0:
        assert not full.any() and not coll.any(), (coll, counts)


def test_strided_cloud_gives_the_same():
    """A cloud that is a view of every other row and column of a larger tensor: all three kernels read it through its strides."""
    for per_grasp in (False, True):
        dense, strided = _run(63, per_grasp, strided=False), _run(63, per_grasp, strided=True)
        for a, b in zip(dense[:4], strided[:4]):
            assert a.tobytes() == b.tobytes(), (per_grasp, a, b)
