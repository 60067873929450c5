"""csrc/depth.hip's depth_normals_kernel against ``icp_projective_reference.image_normals`` on the device: the same bits (NaN
where NaN) at every image shape the lanes and workgroups can divide badly, the jump gate at its threshold, every one-sided
fallback, missing centres, a zero cross product, the orientation, a side stream and every error code."""
import numpy as np
import pytest
import torch

from . import icp_projective_reference as pref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
f32 = np.float32


def gpu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def same_bits(got, want):
    """Equal as bits, any NaN standing for any NaN."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype == np.float32
    nan = np.isnan(want)
    assert (np.isnan(got) == nan).all()
    assert (got.view(np.uint32)[~nan] == want.view(np.uint32)[~nan]).all()


def bumpy(W, H, seed):
    """A smooth slanted surface with a step across it and a few removed pixels: every branch of the kernel at once."""
    rng = np.random.RandomState(seed)
    u, v = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    z = 1.0 + 0.004 * u - 0.003 * v + 0.002 * np.sin(0.7 * u + 0.3 * v) + np.where(u > W / 2, 0.05, 0.0)
    xyz = np.stack([(u - W / 2) / 60.0 * z, (v - H / 2) / 60.0 * z, z], axis=2).reshape(-1, 3).astype(np.float32)
    xyz[rng.rand(W * H) < 0.1] = np.nan
    return xyz


def run(xyz, W, H, step, jump, stream=None):
    from regnet_for_3d_grasping_amd import depth_frame
    return depth_frame.normals(gpu(xyz), W, H, step, jump, stream=stream)


@pytest.mark.parametrize("step", [1, 2])
@pytest.mark.parametrize("shape", [(1, 1), (2, 2), (3, 3), (65, 3), (64, 5)])
def test_the_normals_are_the_restatements_bits(shape, step):
    W, H = shape
    xyz = bumpy(W, H, 100 * W + H)
    got = run(xyz, W, H, step, 0.02).cpu().numpy()
    want = pref.image_normals(xyz, W, H, step, 0.02)
    same_bits(got, want)
    if W * H >= 192:
        assert np.isfinite(want).all(axis=1).sum() > W * H // 3 and np.isnan(want).all(axis=1).sum() > 5


def test_a_step_larger_than_the_image_leaves_every_pixel_without_a_normal():
    xyz = bumpy(64, 5, 1)
    for step in (64, 65, 1 << 40, (1 << 63) - 1):
        assert torch.isnan(run(xyz, 64, 5, step, 0.02)).all()
    same_bits(run(xyz, 64, 5, 5, 0.02).cpu().numpy(), pref.image_normals(xyz, 64, 5, 5, 0.02))     # beyond the height alone


def flat(W=5, H=5):
    u, v = np.meshgrid(np.arange(W), np.arange(H))
    return np.stack([(u - 2) / 64.0, (v - 2) / 64.0, np.ones(u.shape)], axis=2).reshape(-1, 3).astype(np.float32)


def test_the_jump_gate_at_max_jump_and_one_ulp_to_either_side():
    for z, used in ((f32(1.25), True), (np.nextafter(f32(1.25), f32(0)), True), (np.nextafter(f32(1.25), f32(2)), False)):
        xyz = flat()
        xyz[13, 2] = z                                     # the right neighbour of the centre; z - 1 is exact in float32
        got = run(xyz, 5, 5, 1, 0.25).cpu().numpy()
        same_bits(got, pref.image_normals(xyz, 5, 5, 1, 0.25))
        assert (got[12] == np.array([0, 0, -1], dtype=np.float32)).all() != used


@pytest.mark.parametrize("missing", ["left", "right", "up", "down", "left+up", "right+down", "left+right", "up+down"])
@pytest.mark.parametrize("how", ["nan", "border", "jump"])
def test_every_one_sided_fallback(missing, how):
    """The neighbour(s) named are not valid -- NaN, beyond the image, or across a depth jump: the other side against the centre,
    or no normal when both sides of an axis are gone."""
    rng = np.random.RandomState(5)
    W = H = 5
    xyz = flat()
    xyz[:, 2] += (0.01 * rng.rand(25)).astype(np.float32)              # not flat: a one-sided difference gives another normal
    offsets = {"left": (-1, 0), "right": (1, 0), "up": (0, -1), "down": (0, 1)}
    names = missing.split("+")
    if how == "border":
        u = 0 if "left" in names else 4 if "right" in names else 2
        v = 0 if "up" in names else 4 if "down" in names else 2
        if len(names) == 2 and offsets[names[0]][0] == -offsets[names[1]][0] and offsets[names[0]][1] == -offsets[names[1]][1]:
            W, H, xyz = (1, 5, xyz.reshape(5, 5, 3)[:, 2].reshape(-1, 3)) if "left" in names else (5, 1, xyz.reshape(5, 5, 3)[2].reshape(-1, 3))
            u, v = (0, 2) if "left" in names else (2, 0)
    else:
        u = v = 2
        for name in names:
            du, dv = offsets[name]
            xyz[(v + dv) * W + u + du] = np.nan if how == "nan" else xyz[(v + dv) * W + u + du] + np.array([0, 0, 0.5], dtype=np.float32)
    got = run(xyz, W, H, 1, 0.02).cpu().numpy()
    want = pref.image_normals(xyz, W, H, 1, 0.02)
    same_bits(got, want)
    both_gone = missing in ("left+right", "up+down")
    assert np.isnan(want[v * W + u]).all() == both_gone


def test_a_nan_centre_a_zero_cross_product_and_the_orientation():
    xyz = flat()
    xyz[12] = [np.nan, 0.0, 1.0]
    xyz[6, 1] = np.inf
    got = run(xyz, 5, 5, 1, 0.02).cpu().numpy()
    same_bits(got, pref.image_normals(xyz, 5, 5, 1, 0.02))
    assert np.isnan(got[[12, 6]]).all() and got.view(np.uint32)[12].tolist() == [0x7FC00000] * 3
    same = flat()
    same[10:15] = same[12]
    got = run(same, 5, 5, 1, 0.02).cpu().numpy()
    same_bits(got, pref.image_normals(same, 5, 5, 1, 0.02))
    assert np.isnan(got[12]).all()
    huge = flat() * f32(1e30)                                           # len2 overflows: no normal
    assert torch.isnan(run(huge, 5, 5, 1, 3e38)).all() and np.isnan(pref.image_normals(huge, 5, 5, 1, 3e38)).all()
    front, behind = run(flat(), 5, 5, 1, 0.02).cpu().numpy(), run(flat() * f32(-1), 5, 5, 1, 0.02).cpu().numpy()
    assert (front == np.array([0, 0, -1], dtype=np.float32)).all() and (behind == np.array([0, 0, 1], dtype=np.float32)).all()


def test_a_side_stream_gives_the_same_bytes():
    xyz = bumpy(65, 3, 9)
    want = run(xyz, 65, 3, 2, 0.02).cpu().numpy()
    side = torch.cuda.Stream(device=DEV)
    torch.cuda.synchronize()
    got = run(xyz, 65, 3, 2, 0.02, stream=side)
    side.synchronize()
    assert got.cpu().numpy().tobytes() == want.tobytes()


def test_every_error_code():
    from regnet_for_3d_grasping_amd import _lib, depth_frame
    xyz = gpu(flat())
    out = torch.empty_like(xyz)
    stream = torch.cuda.current_stream().cuda_stream
    call = lambda *a: _lib.lib.regnet_depth_normals_f32(*a, stream)    # noqa: E731
    ok = (xyz.data_ptr(), 5, 5, 1, 0.02, out.data_ptr())
    assert call(*ok) == 0
    shape = call(xyz.data_ptr(), 0, 5, 1, 0.02, out.data_ptr())
    assert shape != 0 and shape == call(xyz.data_ptr(), 5, 0, 1, 0.02, out.data_ptr()) == call(xyz.data_ptr(), 5, 5, 0, 0.02, out.data_ptr())
    unsupported = call(xyz.data_ptr(), 1 << 11, (1 << 10) + 1, 1, 0.02, out.data_ptr())
    assert unsupported not in (0, shape)
    for jump in (0.0, -1.0, float("nan"), float("inf"), 1e-60, 1e60):
        assert call(xyz.data_ptr(), 5, 5, 1, jump, out.data_ptr()) == unsupported
    null = call(None, 5, 5, 1, 0.02, out.data_ptr())
    assert null not in (0, shape, unsupported) and null == call(xyz.data_ptr(), 5, 5, 1, 0.02, None)
    assert call(None, 0, 5, 1, float("nan"), None) == shape and call(None, 5, 5, 1, float("nan"), None) == unsupported   # in that order
    with pytest.raises(RuntimeError, match="CUDA"):
        depth_frame.normals(xyz.cpu(), 5, 5)
    with pytest.raises(ValueError, match="rows"):
        depth_frame.normals(xyz, 5, 4)
    with pytest.raises(TypeError):
        depth_frame.normals(xyz.double(), 5, 5)
    with pytest.raises(RuntimeError, match="regnet_depth_normals_f32"):
        depth_frame.normals(xyz, 5, 5, step=0)
    torch.cuda.synchronize()
