"""``GraspDetector`` (regnet_for_3d_grasping_amd/detect.py) end to end: a camera frame in, ``eval_notruth``'s record out, against
the same already-pinned pieces called by hand on the numpy restatement's ``pc`` (tests/ingest_reference.py)."""
import contextlib
import io
import pickle

import numpy as np
import pytest
import torch

from . import ingest_reference as ir
from .test_ingest_cpu import write_pcd

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BOUNDS = (0.5, -0.5, 1.0, 0.5, -0.5)       # the synthetic table (|x| <= 0.4, |y| <= 0.35, z < 0.9) with room to spare
SEED = 1234


def _camera_frame(T):
    """synthetic.make_batch(1000, 1)'s scene lifted into camera coordinates by the inverse transform, colours on the 8-bit
    grid a PCD file holds, padded with 3000 points outside the workspace and 2000 NaN rows, in a seeded order."""
    from regnet_for_3d_grasping_amd import synthetic
    scene = synthetic.make_batch(1000, 1, 25600)[0].numpy().astype(np.float64)
    rng = np.random.RandomState(3)
    outside = np.c_[rng.uniform(0.6, 0.9, 3000), rng.uniform(-0.3, 0.3, 3000), rng.uniform(0.7, 1.5, 3000)]
    outside[1500:, 0] = rng.uniform(-0.3, 0.3, 1500)
    outside[1500:, 2] = rng.uniform(1.1, 1.5, 1500)
    table = np.concatenate([scene[:, :3], outside])
    Tinv = np.linalg.inv(T)
    cam = table @ Tinv[:3, :3].T + Tinv[:3, 3]
    cam = np.concatenate([cam, np.full((2000, 3), np.nan)])
    level = np.concatenate([np.rint(scene[:, 3:6] * 255.0), rng.randint(0, 256, size=(5000, 3))]).astype(np.uint8)
    order = rng.permutation(len(cam))
    cam, level = np.ascontiguousarray(cam[order]), np.ascontiguousarray(level[order])
    t = ir.transform_points(cam, T)
    with np.errstate(invalid="ignore"):
        for col, bound in ((0, BOUNDS[0]), (0, BOUNDS[1]), (2, BOUNDS[2]), (1, BOUNDS[3]), (1, BOUNDS[4])):
            assert not (np.abs(t[:, col] - bound) < 1e-9).any()
    return cam, level.astype(np.float64) / 255.0, level


def _region(net, g, pc, feat, gp):
    with contextlib.redirect_stdout(io.StringIO()), torch.no_grad():
        return net(g[3], g[5], g[2], g[4], g[0], g[1], pc, feat, gp, None, [])


def _same(a, b):
    assert sorted(a) == sorted(b)
    for key in a:
        assert a[key].dtype == b[key].dtype and a[key].shape == b[key].shape, key
        assert a[key].tobytes() == b[key].tobytes(), key


def test_detect_equals_the_pieces_called_by_hand(tmp_path):
    from regnet_for_3d_grasping_amd import detect, eval_collision, ingest, np_random, pipeline, synthetic
    from regnet_for_3d_grasping_amd.get_regiondataset import get_grasp_allobj
    T = ingest.table_frame_transform()
    xyz, rgb, level = _camera_frame(T)
    assert len(xyz) == 30600

    def restated():
        cropped, _ = ir.crop(xyz, rgb, T, BOUNDS)
        assert len(cropped) == 25600                     # the scene, nothing else
        pc, back, color_back = ir.resample(cropped)
        return torch.from_numpy(pc).view(1, 25600, 6).to(DEV), back, color_back

    # ---- models calibrated on the restatement's pc (as tests/test_gpu_testpy_scale.py, on the device)
    np.random.seed(SEED)
    pc, _, _ = restated()
    score_net, region_net = pipeline.build_models(DEV)
    score_net.eval()
    region_net.eval()
    synthetic.calibrate_score_head(score_net, pc)
    with torch.no_grad():
        feat, score, _ = score_net(pc)
    assert int((score > 0.5).sum()) > 4000
    np.random.seed(41)
    got = get_grasp_allobj(pc, score, detect.TEST_PARAMS, [], True)
    np.random.seed(5)
    synthetic.calibrate_region_head(region_net, lambda: _region(region_net, got, pc, feat, detect.GRIPPER_PARAMS))

    # ---- by hand: restatement -> score net -> get_grasp_allobj -> region net -> eval_test, one numpy stream from SEED
    np.random.seed(SEED)
    pc, back, color_back = restated()
    with torch.no_grad():
        feat, score, _ = score_net(pc)
    g = get_grasp_allobj(pc, score, detect.TEST_PARAMS, [], True)
    res = _region(region_net, g, pc, feat, detect.GRIPPER_PARAMS)
    np_random.flush()
    after_hand = int(np.random.randint(0, 2 ** 31 - 1))
    raw = {"grasp_stage2": res[0], "grasp_stage3_stage2": res[8], "grasp_stage3": res[6], "grasp_stage3_score": res[7]}
    points32 = torch.from_numpy(back.astype(np.float32)).to(DEV)
    want = {"points": back, "colors": color_back, "scores": score.view(-1, 1).cpu().numpy()}
    for key, grasp in raw.items():
        assert grasp is not None and grasp.shape[0] >= 1, key            # every set goes through the collision filter
        want[key] = eval_collision.eval_test(points32, grasp[:, :8], None, 0.75, 0.06, 0.08, 0).cpu().numpy()

    # ---- the public call
    detector = detect.GraspDetector(score_net, region_net, bounds=BOUNDS)
    np.random.seed(SEED)
    out = detector.detect((xyz, rgb))
    after = int(np.random.randint(0, 2 ** 31 - 1))
    assert after == after_hand                                            # numpy's stream handed back where the reference leaves it
    assert tuple(out) == detect.RESULT_KEYS
    assert out["points"].dtype == np.float64 and out["points"].shape == (25600, 3)
    assert out["colors"].dtype == np.float64 and out["colors"].shape == (25600, 3)
    assert out["scores"].dtype == np.float32 and out["scores"].shape == (25600, 1)
    for key in raw:
        assert out[key].dtype == np.float32 and out[key].ndim == 2 and out[key].shape[1] == 8, key
        assert detector.raw_counts[key] == raw[key].shape[0] >= 1
    _same(out, want)
    print("detect: stage-2 %d -> %d, stage-3 %d -> %d, stage-3 (score) %d -> %d after the collision filter" % (
        raw["grasp_stage2"].shape[0], len(out["grasp_stage2"]), raw["grasp_stage3"].shape[0], len(out["grasp_stage3"]),
        raw["grasp_stage3_score"].shape[0], len(out["grasp_stage3_score"])))

    # ---- a second call with the same seed: the same bytes
    np.random.seed(SEED)
    _same(detector.detect((xyz, rgb)), out)

    # ---- from a file: PCD in, the pickled record out under the reference's path rule
    folder = tmp_path / "real_data"
    folder.mkdir()
    path = str(folder / "frame.pcd")
    write_pcd(path, xyz, level, "binary_compressed", xyz_type="F8", rgb_type="U4", organised=(170, 180))
    np.random.seed(SEED)
    printed = io.StringIO()
    with contextlib.redirect_stdout(printed):
        from_file, saved = detector.detect_file(path)
    assert saved == str(tmp_path / "real_data_predict" / "frame.p")
    _same(from_file, out)
    with open(saved, "rb") as f:
        _same(pickle.load(f), out)
    lines = printed.getvalue().strip().splitlines()
    assert lines == ["stage2 grasp num: %d" % len(out["grasp_stage2"]), "stage3 grasp num: %d" % len(out["grasp_stage2"]),
                     "stage3 grasp num (with scorethre): %d" % len(out["grasp_stage3_score"])]

    # ---- a dataset record (.p): no transform, no crop; float32 points in the record
    record = {"view_cloud": back.astype(np.float32), "view_cloud_color": color_back.astype(np.float32)}
    rec_path = str(tmp_path / "virtual_data" / "scene.p")
    (tmp_path / "virtual_data").mkdir()
    with open(rec_path, "wb") as f:
        pickle.dump(record, f, protocol=2)
    np.random.seed(SEED)
    with contextlib.redirect_stdout(io.StringIO()):
        rec_out, rec_saved = detector.detect_file(rec_path)
    assert rec_saved == str(tmp_path / "virtual_data_predict" / "scene.p")
    assert rec_out["points"].dtype == np.float32 and rec_out["points"].tobytes() == record["view_cloud"].tobytes()
    assert rec_out["scores"].shape == (25600, 1) and rec_out["grasp_stage2"].shape[1] == 8
