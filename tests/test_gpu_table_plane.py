"""Table-plane estimation on the device (csrc/plane.hip, table_plane.py) against the numpy restatement of its contract
(tests/plane_reference.py): the hypothesis table bit for bit, every count, the winner and the inlier mask exactly; the float64
moments within the worst-case summation bound; and ``GraspDetector(transform="auto")`` end to end."""
import contextlib
import io
import math
import pickle

import numpy as np
import pytest
import torch

from . import plane_reference as ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
RANGE = (0.5, 1.2)
SEED = 1234


def _cloud(M, seed, dtype=np.float32):
    """A tilted plane with 2 mm noise (60 %), clutter (25 %) and NaN / infinite rows (15 %), in a seeded order."""
    rng = np.random.RandomState(seed)
    u, v = rng.uniform(-0.5, 0.5, M), rng.uniform(-0.4, 0.4, M)
    pts = np.stack([u, v, 1.0 + 0.3 * u - 0.2 * v + rng.normal(0, 0.002, M)], axis=1)
    kind = rng.rand(M)
    clutter = kind < 0.25
    pts[clutter] = rng.uniform(-0.6, 0.6, (int(clutter.sum()), 3)) + [0, 0, 1.0]
    pts[kind > 0.90] = np.nan
    pts[(kind > 0.85) & (kind <= 0.87), 1] = np.inf
    if dtype == np.float64:
        pts[(kind > 0.87) & (kind <= 0.88), 2] = 1e300         # finite in float64, infinite once rounded to float32
    return np.ascontiguousarray(pts.astype(dtype))


def _device(xyz, **kw):
    from regnet_for_3d_grasping_amd import table_plane
    t = torch.from_numpy(np.ascontiguousarray(xyz)).to(DEV)
    result, details, _ = table_plane.estimate_device(t, **kw)
    torch.cuda.synchronize()
    host = result.cpu().numpy()
    return {"table": details.hypotheses.cpu().numpy(), "counts": details.counts.cpu().numpy(),
            "mask": details.inlier_mask.cpu().numpy(), "moments": host[:80].view(np.float64).copy(),
            "winner": int(host[80:84].view(np.int32)[0]), "count": int(host[84:88].view(np.int32)[0])}


def _check(xyz, threshold=0.005, hypotheses=1024, seed=0, range=(0.0, math.inf), up_hint=None, max_tilt_deg=None, got=None):
    want = ref.estimate_plane(xyz, threshold, hypotheses, seed, range, up_hint, max_tilt_deg)
    if got is None:
        got = _device(xyz, threshold=threshold, hypotheses=hypotheses, seed=seed, range=range, up_hint=up_hint,
                      max_tilt_deg=max_tilt_deg)
    assert got["table"].dtype == np.float32 and got["table"].shape == (hypotheses, 8)
    assert got["table"].tobytes() == want["table"].tobytes()                      # bit for bit (also the sign of a zero)
    assert got["counts"].dtype == np.int32 and np.array_equal(got["counts"], want["counts"])
    assert got["winner"] == want["winner"] and got["count"] == want["count"]
    assert got["mask"].dtype == np.uint8 and np.array_equal(got["mask"].astype(bool), want["mask"])
    if want["winner"] < 0:
        assert (got["moments"] == 0).all()
        return got, want
    # the float64 sums in any order: both this sum and numpy's are within n 2^-53 sum|term| of each other (the worst-case
    # error of a sum of n exact terms in any order is (n - 1) u sum|term|, u = 2^-53)
    n = want["count"]
    bound = n * 2.0 ** -53 * want["abs_moments"]
    error = np.abs(got["moments"] - want["moments"])
    print("moments: n = %d, largest error / bound = %.3g" % (n, (error / np.maximum(bound, 1e-300)).max()))
    assert got["moments"][0] == n and (error <= bound).all()
    # the normal: a perturbation E of the covariance turns the smallest eigenvector by at most 2 |E| / gap (Davis-Kahan);
    # |E| from the moments' bounds through C = S / n - c c^T
    from regnet_for_3d_grasping_amd import table_plane
    plane = table_plane.plane_from_moments(got["moments"], got["winner"], got["count"])
    c_abs = np.abs(want["moments"][1:4]) / n
    dS, dc = bound[4:].max() / n, bound[1:4].max() / n
    E = 3.0 * (dS + 2.0 * c_abs.max() * dc + dc * dc) + 1e-15 * (want["abs_moments"][4:].max() / n)   # + eigh's own rounding
    gap = want["eigenvalues"][1] - want["eigenvalues"][0]
    if gap > 1e3 * E:
        angle = math.asin(min(1.0, float(np.linalg.norm(np.cross(plane.normal, want["normal"])))))   # (exact for small angles)
        limit = 2.0 * E / gap
        print("normal: angle %.3g rad, limit %.3g rad" % (angle, limit))
        assert angle <= limit
        assert float(plane.normal @ want["normal"]) > 0 and abs(plane.offset - want["offset"]) <= limit * 4.0 + 1e-9
    return got, want


@pytest.fixture(scope="module")
def frame32():
    return ref.synthetic_frame()[0]


@pytest.mark.parametrize("hypotheses", [1024, 4096])
def test_synthetic_frame_float32(frame32, hypotheses):
    got, want = _check(frame32, hypotheses=hypotheses, range=RANGE)
    assert (got["table"][:, 7] >= 1.0).all()                   # every slot filled under the retry rule
    if hypotheses == 1024:
        assert got["winner"] == 970 and got["count"] == 84345
    plain, _ = _check(frame32, hypotheses=1024)
    assert plain["count"] == 125454                            # ungated, the floor wins


def test_synthetic_frame_float64():
    xyz = ref.synthetic_frame(dtype=np.float64)[0]
    assert xyz.dtype == np.float64 and (xyz[np.isfinite(xyz)].astype(np.float32).astype(np.float64) != xyz[np.isfinite(xyz)]).any()
    got, _ = _check(xyz, range=RANGE)
    same = _device(xyz.astype(np.float32), range=RANGE)        # rounded once: the float32 frame gives the same bits
    for key in ("table", "counts", "mask"):
        assert got[key].tobytes() == same[key].tobytes()


@pytest.mark.parametrize("M", [1, 2, 3, 63, 64, 65, 2047, 2048, 2049, 100003])
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_sizes(M, dtype):
    got, want = _check(_cloud(M, M, dtype), hypotheses=256 if M > 1000 else 64, seed=M % 7)
    if M >= 63:
        assert want["winner"] >= 0
    if M == 1:
        assert want["winner"] == -1 and (got["table"][:, 7] == 0).all()


def test_largest_frame():
    xyz = _cloud(1 << 21, 21)
    _check(xyz, hypotheses=64, seed=3)
    from regnet_for_3d_grasping_amd import table_plane
    with pytest.raises(ValueError):
        table_plane.estimate_device(torch.zeros(((1 << 21) + 1, 3), device=DEV))


@pytest.mark.parametrize("hypotheses", [64, 128, 192, 1024, 4096])
def test_hypothesis_counts(hypotheses):
    _check(_cloud(20011, 5), hypotheses=hypotheses, seed=2)


@pytest.mark.parametrize("seed", [0, 1, 2, 12345, 2 ** 32 - 1])
def test_seeds(seed):
    got, _ = _check(_cloud(30000, 9), hypotheses=128, seed=seed)
    if seed:
        first, _ = _check(_cloud(30000, 9), hypotheses=128, seed=0)
        assert got["table"].tobytes() != first["table"].tobytes()


def test_empty_all_nan_and_duplicated_points():
    from regnet_for_3d_grasping_amd import table_plane
    got, want = _check(np.zeros((0, 3), dtype=np.float32), hypotheses=64)
    assert got["winner"] == -1 and got["count"] == 0 and (got["counts"] == -1).all()
    got, _ = _check(np.full((5000, 3), np.nan, dtype=np.float32), hypotheses=128)
    assert got["winner"] == -1 and not got["table"].any() and not got["mask"].any()
    got, _ = _check(np.full((5000, 3), np.inf, dtype=np.float64), hypotheses=128)
    assert got["winner"] == -1
    got, _ = _check(np.tile(np.array([[0.25, -0.5, 1.0]], dtype=np.float32), (5000, 1)), hypotheses=128)
    assert got["winner"] == -1 and (got["table"][:, 7] == 0).all() and (got["table"][:, 3] == 0.25).all()
    # a cloud of which half the rows are copies of one point: its triples are invalid, the rest finds the plane
    xyz = _cloud(20000, 4)
    xyz[::2] = xyz[1]
    got, want = _check(xyz, hypotheses=256)
    assert want["winner"] >= 0 and (got["table"][:, 7] == 0).any()
    for bad in (np.full((100, 3), np.nan, dtype=np.float32), np.zeros((0, 3), dtype=np.float32)):
        with pytest.raises(ValueError, match="no plane"):
            table_plane.estimate_plane(bad, device=DEV)


def test_gates(frame32):
    xyz = frame32[::3]
    for kw in ({"range": (1.2, 2.0)}, {"range": (0.0, 0.3)}, {"range": RANGE, "up_hint": (0.0, -0.4, -0.9), "max_tilt_deg": 10.0},
               {"up_hint": (1.0, 0.0, 0.0), "max_tilt_deg": 20.0}, {"up_hint": (0.0, 0.0, -2.5), "max_tilt_deg": 45.0},
               {"range": (0.9, 0.92)}, {"threshold": 0.001, "range": RANGE}, {"threshold": 0.05}):
        got, want = _check(xyz, hypotheses=512, seed=1, **kw)
        print(kw, "->", want["winner"], want["count"], int((want["table"][:, 7] == 2).sum()), "eligible")
    # no plane through a point of the frame is farther from the camera than that point: nothing is eligible
    got, want = _check(xyz, hypotheses=512, seed=1, range=(5.0, 9.0))
    assert want["winner"] == -1 and (got["counts"] == -1).all() and (got["table"][:, 7] == 1.0).all()


def test_non_default_stream_and_repeat(frame32):
    from regnet_for_3d_grasping_amd import table_plane
    first = _device(frame32, range=RANGE)
    second = _device(frame32, range=RANGE)
    for key in ("table", "counts", "mask"):
        assert first[key].tobytes() == second[key].tobytes()
    assert (first["winner"], first["count"]) == (second["winner"], second["count"])
    side = torch.cuda.Stream(device=DEV)
    t = torch.from_numpy(frame32).to(DEV)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        result, details, _ = table_plane.estimate_device(t, range=RANGE)
    side.synchronize()
    got = {"table": details.hypotheses.cpu().numpy(), "counts": details.counts.cpu().numpy(),
           "mask": details.inlier_mask.cpu().numpy()}
    for key in got:
        assert got[key].tobytes() == first[key].tobytes()
    assert result.cpu().numpy()[80:88].tobytes() == np.array([first["winner"], first["count"]], dtype=np.int32).tobytes()


def test_estimate_plane_and_calibrate(frame32):
    from regnet_for_3d_grasping_amd import ingest, table_plane
    want = ref.estimate_plane(frame32, range=RANGE)
    for source in (frame32, torch.from_numpy(frame32), torch.from_numpy(frame32).to(DEV)):
        plane, details = table_plane.estimate_plane(source, range=RANGE, return_details=True, device=DEV)
        assert plane.hypothesis == want["winner"] and plane.inliers == want["count"]
        # (the moments' worst-case bound moves the covariance by < 1e-10: the normal by < 3e-9, the rms by < 1e-10 / (2 rms))
        assert abs(plane.rms - want["rms"]) < 1e-7 and np.abs(plane.normal - want["normal"]).max() < 1e-8
        assert details.counts.is_cuda and details.hypotheses.is_cuda and details.inlier_mask.is_cuda
        assert np.array_equal(details.counts.cpu().numpy(), want["counts"])
    state = np.random.get_state()
    T, plane = table_plane.calibrate(frame32, range=RANGE, device=DEV)
    after = np.random.get_state()
    assert state[2] == after[2] and np.array_equal(state[1], after[1])          # numpy's global stream is not touched
    assert np.abs(T - ref.table_frame(want["normal"], want["offset"])).max() < 1e-8
    error = np.abs(T - ingest.table_frame_transform())
    # (the bounds of tests/test_table_plane_cpu.py: twice what the restatement achieves on this seed, plus the 1e-8 above)
    assert error[:3, :3].max() < 2 * 3.0004e-05 + 1e-8 and error[:3, 3].max() < 2 * 4.359e-07 + 1e-8
    with pytest.raises(ValueError):
        table_plane.estimate_plane(frame32, hypotheses=100, device=DEV)
    with pytest.raises(ValueError):
        table_plane.estimate_plane(frame32, up_hint=(0, 0, 1), device=DEV)


# ---- the detector ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def detector_parts():
    """Networks calibrated on the synthetic frame's own cropped cloud (the recipe of tests/test_gpu_detect.py)."""
    from regnet_for_3d_grasping_amd import detect, np_random, pipeline, synthetic
    from regnet_for_3d_grasping_amd.get_regiondataset import get_grasp_allobj
    from . import test_gpu_detect as td
    xyz, rgb = ref.synthetic_frame(dtype=np.float64)
    score_net, region_net = pipeline.build_models(DEV)
    score_net.eval()
    region_net.eval()
    probe = detect.GraspDetector(score_net, region_net)
    np.random.seed(SEED)
    with np_random.deferred(), torch.no_grad():
        pc = probe.ingest((xyz, rgb)).pc.clone()
    synthetic.calibrate_score_head(score_net, pc)
    with torch.no_grad():
        feat, score, _ = score_net(pc)
    np.random.seed(41)
    got = get_grasp_allobj(pc, score, detect.TEST_PARAMS, [], True)
    np.random.seed(5)
    synthetic.calibrate_region_head(region_net, lambda: td._region(region_net, got, pc, feat, detect.GRIPPER_PARAMS))
    return score_net, region_net, (xyz, rgb)


def _run(parts, **kw):
    from regnet_for_3d_grasping_amd import detect
    score_net, region_net, frame = parts
    detector = detect.GraspDetector(score_net, region_net, **kw)
    np.random.seed(SEED)
    out = detector.detect(frame)
    state = np.random.get_state()
    return detector, out, state


def _same_state(a, b):
    return a[0] == b[0] and np.array_equal(a[1], b[1]) and a[2:] == b[2:]


def test_detector_auto_equals_the_estimated_transform_given_explicitly(detector_parts):
    from regnet_for_3d_grasping_amd import detect, table_plane
    auto, out, state = _run(detector_parts, transform={"range": RANGE})
    assert tuple(out) == detect.RESULT_KEYS + detect.TABLE_KEYS
    T, summary = out["table_transform"], out["table_plane"]
    assert T.dtype == np.float64 and T.shape == (4, 4) and summary.dtype == np.float64 and summary.shape == (5,)
    plane = table_plane.estimate_plane(detector_parts[2][0], range=RANGE, device=DEV)
    # (a second estimate: the float64 moments are summed in another order, everything else is the same)
    assert np.abs(summary - np.array(list(plane.normal) + [plane.offset, plane.rms])).max() < 1e-7
    assert np.array_equal(T, table_plane.table_frame((summary[:3], summary[3]), 0.75))
    assert np.abs(T - ref.default_transform())[:3, :3].max() < 2 * 3.0004e-05 + 1e-8
    assert len(out["points"]) > 20000
    print("auto: %d points kept, %d / %d / %d grasps" % (len(out["points"]), len(out["grasp_stage2"]), len(out["grasp_stage3"]),
                                                         len(out["grasp_stage3_score"])))
    explicit, want, want_state = _run(detector_parts, transform=T)
    assert tuple(want) == detect.RESULT_KEYS
    for key in detect.RESULT_KEYS:
        assert out[key].dtype == want[key].dtype and np.array_equal(out[key], want[key]), key
    assert _same_state(state, want_state)                      # numpy's generator: consumed exactly as without the estimate
    # with selection the table keys come last; "auto" as a word = no keyword given
    _, selected, _ = _run(detector_parts, transform={"range": RANGE}, select={"top_k": 5})
    assert tuple(selected) == detect.RESULT_KEYS + detect.SELECT_KEYS + detect.TABLE_KEYS
    assert detect.GraspDetector(detector_parts[0], detector_parts[1], transform="auto").auto_table == {}
    with pytest.raises(ValueError):
        detect.GraspDetector(detector_parts[0], detector_parts[1], transform="automatic")
    # calibrate once, then detect with the fixed transform
    fixed = detect.GraspDetector(detector_parts[0], detector_parts[1], transform={"range": RANGE})
    T_fixed, _ = fixed.calibrate(detector_parts[2])
    assert np.abs(T_fixed - T).max() < 1e-8 and fixed.auto_table is None and fixed.transform is T_fixed
    np.random.seed(SEED)
    again = fixed.detect(detector_parts[2])
    assert tuple(again) == detect.RESULT_KEYS
    _, same, _ = _run(detector_parts, transform=T_fixed)
    for key in detect.RESULT_KEYS:
        assert np.array_equal(again[key], same[key]), key
    # a dataset record is never transformed: no table keys
    record = {"view_cloud": want["points"].astype(np.float32), "view_cloud_color": want["colors"].astype(np.float32)}
    np.random.seed(SEED)
    assert tuple(auto.detect(record)) == detect.RESULT_KEYS


def test_default_detector_is_unchanged(detector_parts):
    from regnet_for_3d_grasping_amd import detect, ingest
    _, plain, plain_state = _run(detector_parts)
    _, explicit, explicit_state = _run(detector_parts, transform=ingest.table_frame_transform())
    assert tuple(plain) == tuple(explicit) == detect.RESULT_KEYS
    for key in detect.RESULT_KEYS:
        assert plain[key].dtype == explicit[key].dtype and plain[key].tobytes() == explicit[key].tobytes(), key
    assert _same_state(plain_state, explicit_state)


def test_cli_auto_table_writes_the_two_extra_keys(detector_parts, tmp_path):
    import argparse
    from regnet_for_3d_grasping_amd import detect
    from .test_ingest_cpu import write_pcd
    score_net, region_net, (xyz, rgb) = detector_parts
    folder = tmp_path / "real_data"
    folder.mkdir()
    path = str(folder / "frame.pcd")
    write_pcd(path, xyz, np.rint(rgb * 255.0).astype(np.uint8), "binary", xyz_type="F8", rgb_type="U4", organised=(640, 480))
    flags = argparse.Namespace(auto_table=True, table_range=list(RANGE), plane_threshold=None)
    records = []
    for transform in (detect.transform_from_args(flags), None):
        detector = detect.GraspDetector(score_net, region_net, transform=transform)
        if transform is None:
            detector.transform = records[0]["table_transform"]
        np.random.seed(SEED)
        printed = io.StringIO()
        with contextlib.redirect_stdout(printed):
            _, saved = detector.detect_file(path)
        assert saved == str(tmp_path / "real_data_predict" / "frame.p") and len(printed.getvalue().strip().splitlines()) == 3
        with open(saved, "rb") as f:
            records.append(pickle.load(f))
    with_table, without = records
    assert tuple(with_table) == detect.RESULT_KEYS + detect.TABLE_KEYS and tuple(without) == detect.RESULT_KEYS
    for key in detect.RESULT_KEYS:
        assert with_table[key].tobytes() == without[key].tobytes(), key
