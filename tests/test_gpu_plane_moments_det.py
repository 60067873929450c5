"""The fixed-order moments of the table plane on the device (csrc/plane.hip, table_plane.moments_fixed_order): within the
worst-case summation bound of the float64 reference, the same bits on every call, and ``estimate_plane`` with them."""
import numpy as np
import pytest
import torch

from . import plane_reference as ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _cloud(M, seed, dtype):
    rng = np.random.RandomState(seed)
    xyz = rng.uniform(-1.0, 1.0, (M, 3)) + [0.0, 0.0, 1.5]
    xyz[rng.rand(M) < 0.05] = np.nan
    xyz[rng.rand(M) < 0.01, 1] = np.inf
    return np.ascontiguousarray(xyz.astype(dtype)), (rng.rand(M) < 0.6).astype(np.uint8)


@pytest.mark.parametrize("M", [0, 1, 2047, 2048, 2049, 100003, 1 << 21])
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_against_the_reference_and_repeatable(M, dtype):
    from regnet_for_3d_grasping_amd import table_plane
    xyz, mask = _cloud(M, M % 97, dtype)
    p, finite = ref.to_f32(xyz)
    want, want_abs = ref.moments_of(p, mask.astype(bool) & finite)
    xyz_d, mask_d = torch.from_numpy(xyz).to(DEV), torch.from_numpy(mask).to(DEV)
    runs = [table_plane.moments_fixed_order(xyz_d, mask_d).cpu().numpy() for _ in range(3)]
    assert runs[0].dtype == np.float64 and runs[0].shape == (10,)
    assert runs[0].tobytes() == runs[1].tobytes() == runs[2].tobytes()
    # a sum of n exact terms in any order is within (n - 1) u sum|term| of the exact sum, u = 2^-53: twice that between two sums
    n = int(want[0])
    assert runs[0][0] == n and (np.abs(runs[0] - want) <= 2.0 * n * 2.0 ** -53 * want_abs).all()


def test_estimate_plane_twice_gives_the_same_bits():
    from regnet_for_3d_grasping_amd import table_plane
    xyz = ref.synthetic_frame()[0]
    first = table_plane.estimate_plane(xyz, range=(0.5, 1.2), device=DEV)
    for source in (xyz, torch.from_numpy(xyz).to(DEV)):
        again = table_plane.estimate_plane(source, range=(0.5, 1.2), device=DEV)
        assert again.normal.tobytes() == first.normal.tobytes() and again.offset == first.offset and again.rms == first.rms
    want = ref.estimate_plane(xyz, range=(0.5, 1.2))
    assert first.hypothesis == want["winner"] and first.inliers == want["count"]
    assert abs(first.rms - want["rms"]) < 1e-7 and np.abs(first.normal - want["normal"]).max() < 1e-8
