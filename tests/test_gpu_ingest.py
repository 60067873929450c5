"""The device front end of single-file inference (csrc/ingest.hip, regnet_for_3d_grasping_amd/ingest.py) against the numpy
restatement of test.py:112-127 (tests/ingest_reference.py) and against the fixture the reference's own utils.noise_color +
np.random.choice produced (tests/golden/s10_ingest.npz).  Every comparison is exact."""
import hashlib
import os

import numpy as np
import pytest
import torch

from . import ingest_reference as ir

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "s10_ingest.npz")


def _crop_and_compare(xyz, rgb, T, bounds=ir.DEFAULT_BOUNDS, drop_nonfinite=True):
    """Run the crop kernel on (xyz, rgb) as given (float32 or float64) and require the restatement's rows, no row left out."""
    from regnet_for_3d_grasping_amd import ingest
    want, want_src = ir.crop(xyz, rgb, T, bounds, drop_nonfinite)
    k64, k32, krgb, count, src = ingest.crop_frame(torch.from_numpy(xyz).to(DEV), torch.from_numpy(rgb).to(DEV), T, bounds,
                                                   drop_nonfinite, with_source=True)
    assert count.is_cuda and count.dtype == torch.int32
    n = int(count.cpu())
    assert n == len(want)
    assert np.array_equal(src[:n].cpu().numpy(), want_src)
    assert k64[:n].cpu().numpy().tobytes() == np.ascontiguousarray(want[:, :3]).tobytes()
    assert k32[:n].cpu().numpy().tobytes() == want[:, :3].astype(np.float32).tobytes()
    assert krgb[:n].cpu().numpy().tobytes() == np.ascontiguousarray(want[:, 3:6]).tobytes()
    return n


# ---- 4. regnet_ingest_crop ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_crop_organised_frame_with_holes(dtype):
    from regnet_for_3d_grasping_amd import ingest
    T = ingest.table_frame_transform()
    xyz, rgb = ir.camera_frame(11, 640 * 480, T)
    if dtype == np.float32:
        # the float32 frame is its own input (widened exactly by the kernel): clear the margins for ITS coordinates
        xyz = xyz.astype(np.float32)
        t = ir.transform_points(xyz, T)
        with np.errstate(invalid="ignore"):
            near = np.zeros(len(xyz), dtype=bool)
            for col, bound in ((0, 0.26), (0, -0.4), (2, 1.0), (1, 0.65), (1, 0.2)):
                near |= np.abs(t[:, col] - bound) < 1e-9
        xyz[near] = np.float32(5.0)                    # far outside every bound
        rgb = rgb.astype(np.float32)
    assert 0.25 < np.isnan(xyz[:, 0]).mean() < 0.35
    n = _crop_and_compare(xyz, rgb, T)
    assert 25600 < n < len(xyz) // 2


def test_crop_everything_and_nothing_kept():
    T = np.eye(4)
    rng = np.random.RandomState(5)
    xyz = rng.uniform(-1, 1, size=(10000, 3))
    rgb = rng.rand(10000, 3)
    assert _crop_and_compare(xyz, rgb, T, (2.0, -2.0, 2.0, 2.0, -2.0)) == 10000
    assert _crop_and_compare(xyz, rgb, T, (np.inf, -np.inf, np.inf, np.inf, -np.inf)) == 10000
    assert _crop_and_compare(xyz, rgb, T, (-2.0, -3.0, 2.0, 2.0, -2.0)) == 0
    assert _crop_and_compare(np.full((777, 3), np.nan), rng.rand(777, 3), T) == 0


@pytest.mark.parametrize("M", [0, 1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025])
def test_crop_small_sizes(M):
    from regnet_for_3d_grasping_amd import ingest
    T = ingest.table_frame_transform()
    xyz, rgb = ir.camera_frame(100 + M, M, T, nan_fraction=0.1)
    n = _crop_and_compare(xyz, rgb, T)
    assert 0 <= n <= M


def test_crop_points_on_the_bounds_are_dropped():
    """Rows exactly ON each bound (identity transform, so the coordinate IS the bound) fail the strict tests; their
    neighbours one ulp inside pass.  An infinite coordinate never survives, with or without drop_nonfinite: it reaches x as
    0 * inf = NaN or as an infinity, and both fail a strict two-sided test."""
    T = np.eye(4)
    x_hi, x_lo, z_hi, y_hi, y_lo = ir.DEFAULT_BOUNDS
    inside = np.array([0.0, 0.4, 0.5])
    rows = []
    for col, bound, inward in ((0, x_hi, -1), (0, x_lo, 1), (2, z_hi, -1), (1, y_hi, -1), (1, y_lo, 1)):
        on, near = inside.copy(), inside.copy()
        on[col] = bound
        near[col] = np.nextafter(bound, bound + inward)
        rows += [on, near]
    rows.append(np.array([0.0, 0.4, -np.inf]))
    xyz = np.tile(np.array(rows), (40, 1))             # several workgroups, on-bound rows at varying lanes
    rgb = np.random.RandomState(1).rand(len(xyz), 3)
    assert _crop_and_compare(xyz, rgb, T, drop_nonfinite=True) == 5 * 40
    assert _crop_and_compare(xyz, rgb, T, drop_nonfinite=False) == 5 * 40


def test_crop_rejects_oversized_frames_and_cpu_tensors():
    from regnet_for_3d_grasping_amd import ingest
    with pytest.raises(RuntimeError, match="CUDA tensor"):
        ingest.crop_frame(torch.zeros(4, 3), torch.zeros(4, 3), np.eye(4))
    with pytest.raises(TypeError):
        ingest.crop_frame(torch.zeros(4, 3, device=DEV), torch.zeros(4, 3, device=DEV, dtype=torch.float64), np.eye(4))


# ---- 5. ingest_frame / ingest_record ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,cloud_seed,num_points,seed", ir.FIXTURE_CASES)
def test_ingest_record_equals_the_reference_fixture(name, cloud_seed, num_points, seed):
    """The ``.p`` branch: float32 arrays, noise_color, choice -- against what the reference itself computed."""
    from regnet_for_3d_grasping_amd import ingest, np_random
    gold = np.load(GOLDEN)
    key = "%s_f32_" % name
    xyz, rgb, _ = ir.record_cloud(cloud_seed, num_points)
    np.random.seed(seed)
    fr = ingest.ingest_record({"view_cloud": xyz, "view_cloud_color": rgb}, device=DEV)
    np_random.flush()
    state = np.random.get_state()
    pc = fr.pc.cpu().numpy()
    assert pc.shape == (1, 25600, 6) and pc.dtype == np.float32
    assert hashlib.sha256(pc.tobytes()).digest() == gold[key + "pc_sha256"].tobytes()
    assert np.array_equal(state[1], gold[key + "state_key"]) and int(state[2]) == int(gold[key + "state_pos"])
    back, color_back = fr.download()
    assert back.dtype == np.float32 and back.tobytes() == xyz.astype(np.float32).tobytes()
    assert color_back.tobytes() == rgb.astype(np.float32).tobytes()


@pytest.mark.parametrize("name,cloud_seed,num_points,seed", ir.FIXTURE_CASES)
def test_ingest_frame_equals_the_reference_fixture(name, cloud_seed, num_points, seed):
    """The ``real_data`` branch's float64 array (identity transform, open bounds: every row kept, as the fixture's)."""
    from regnet_for_3d_grasping_amd import ingest, np_random
    gold = np.load(GOLDEN)
    key = "%s_f64_" % name
    xyz, rgb, _ = ir.record_cloud(cloud_seed, num_points)
    np.random.seed(seed)
    fr = ingest.ingest_frame(xyz, rgb, np.eye(4), (np.inf, -np.inf, np.inf, np.inf, -np.inf), device=DEV)
    np_random.flush()
    state = np.random.get_state()
    # x * 1 + y * 0 + z * 0 + 0 is x exactly: the identity transform leaves the fixture's float64 coordinates
    pc = fr.pc.cpu().numpy()
    assert hashlib.sha256(pc.tobytes()).digest() == gold[key + "pc_sha256"].tobytes()
    assert np.array_equal(state[1], gold[key + "state_key"]) and int(state[2]) == int(gold[key + "state_pos"])
    back, color_back = fr.download()
    assert back.dtype == np.float64 and back.tobytes() == xyz.tobytes() and color_back.tobytes() == rgb.tobytes()


@pytest.mark.parametrize("frame_seed,num_points,expect_replace", [(21, 640 * 480, False), (22, 60000, True)])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_ingest_frame_equals_the_restatement(frame_seed, num_points, expect_replace, dtype):
    """Transformed + cropped frames, both resampling modes (kept count above and below 25 600), same numpy seed on both sides."""
    from regnet_for_3d_grasping_amd import ingest, np_random
    T = ingest.table_frame_transform()
    xyz, rgb = ir.camera_frame(frame_seed, num_points, T, margin=1e-6)    # (1e-6: the float32 frame's coordinates move by < 1e-7)
    xyz, rgb = xyz.astype(dtype), rgb.astype(dtype)
    np.random.seed(77)
    cropped, _ = ir.crop(xyz, rgb, T)
    assert (len(cropped) < 25600) == expect_replace and len(cropped) > 1000
    want, want_back, want_color = ir.resample(cropped)
    want_after = int(np.random.randint(0, 2 ** 31 - 1))
    np.random.seed(77)
    fr = ingest.ingest_frame(xyz, rgb, device=DEV)
    np_random.flush()
    after = int(np.random.randint(0, 2 ** 31 - 1))
    assert fr.pc.cpu().numpy().tobytes() == want.reshape(1, 25600, 6).tobytes()
    assert after == want_after
    back, color_back = fr.download()
    assert back.dtype == np.float64 and back.tobytes() == want_back.tobytes() and color_back.tobytes() == want_color.tobytes()
    assert int(fr.count.cpu()) == len(cropped)


def test_ingest_frame_empty_workspace_raises_at_the_read():
    from regnet_for_3d_grasping_amd import ingest, np_random
    xyz = np.full((500, 3), 9.0)
    fr = ingest.ingest_frame(xyz, np.zeros((500, 3)), np.eye(4), device=DEV)
    np_random.flush()
    assert int(fr.count.cpu()) == 0 and not fr.pc.cpu().numpy().any()
    with pytest.raises(ValueError):
        fr.download()


# ---- 7. no hidden synchronisation -----------------------------------------------------------------------------------------
def test_ingest_frame_does_not_synchronise():
    """With the frame on the device and numpy's generator state resident there (a first call has handed it over), a call
    enqueues work and returns: torch's sync debug mode turns any blocking call into an error."""
    from regnet_for_3d_grasping_amd import ingest, np_random
    T = ingest.table_frame_transform()
    xyz, rgb = ir.camera_frame(31, 640 * 480, T)
    xyz_d, rgb_d = torch.from_numpy(xyz).to(DEV), torch.from_numpy(rgb).to(DEV)
    np.random.seed(9)
    want1, _, _ = ir.resample(ir.crop(xyz, rgb, T)[0])
    want2, _, _ = ir.resample(ir.crop(xyz, rgb, T)[0])
    np.random.seed(9)
    with np_random.deferred():
        first = ingest.ingest_frame(xyz_d, rgb_d, device=DEV)
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")
        try:
            fr = ingest.ingest_frame(xyz_d, rgb_d, device=DEV)
        finally:
            torch.cuda.set_sync_debug_mode("default")
        assert fr.count.is_cuda and fr.count.dtype == torch.int32 and fr.pc.is_cuda
    assert first.pc.cpu().numpy().tobytes() == want1.reshape(1, 25600, 6).tobytes()
    assert fr.pc.cpu().numpy().tobytes() == want2.reshape(1, 25600, 6).tobytes()
