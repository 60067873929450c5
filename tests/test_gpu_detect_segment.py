"""``GraspDetector(segment=...)`` end to end on a synthetic frame with three separated boxes on a table: the record's
``SEGMENT_KEYS`` against the numpy restatement (tests/cluster_reference.py) run on the record's own points, the per-object
selection, the unchanged default record and the CLI flags.  Box tops without sides leave no grasp after the collision filter, so
the grasp assignment and the per-object selection run on a second frame, synthetic.make_batch's scene, where grasps survive."""
import argparse
import contextlib
import io
import pickle

import numpy as np
import pytest
import torch

from . import cluster_reference as ref
from . import plane_reference

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SEED = 1234
SCENE_BOUNDS = (0.5, -0.5, 1.0, 0.5, -0.5)  # synthetic.make_batch's table with room to spare (tests/test_gpu_detect.py)
BOXES = ((-0.2, 0.3, 0.05, 0.1), (0.0, 0.45, 0.05, 0.15), (0.1, 0.25, 0.04, 0.05))     # centre x, y, half width, height


def _frame(seed=5, width=640, height=480, noise=0.0015, holes=0.3):
    """plane_reference.synthetic_frame's table and floor with the three boxes above, far more than a tolerance apart."""
    rng = np.random.RandomState(seed)
    n = width * height
    x, y = rng.uniform(-0.9, 0.8, n), rng.uniform(-0.2, 1.2, n)
    z = np.where((x > -0.6) & (x < 0.5) & (y > 0) & (y < 0.9), 0.75, 0.0)
    for cx, cy, half, tall in BOXES:
        z[(np.abs(x - cx) < half) & (np.abs(y - cy) < half)] = 0.75 + tall
    z = z + rng.normal(0, noise, n)
    cam = np.c_[x, y, z, np.ones(n)] @ np.linalg.inv(plane_reference.default_transform()).T
    xyz = cam[:, :3].copy()
    xyz[rng.rand(n) < holes] = np.nan
    rgb = rng.randint(0, 256, size=(n, 3)).astype(np.float64) / 255.0
    return np.ascontiguousarray(xyz), rgb


def _region(net, g, pc, feat, gp):
    with contextlib.redirect_stdout(io.StringIO()), torch.no_grad():
        return net(g[3], g[5], g[2], g[4], g[0], g[1], pc, feat, gp, None, [])


def _scene_frame():
    """synthetic.make_batch(1000, 1)'s scene -- objects with sides, on which grasps survive the collision filter -- lifted into
    camera coordinates, colours on the 8-bit grid (the frame of tests/test_gpu_detect.py without its padding)."""
    from regnet_for_3d_grasping_amd import ingest, synthetic
    scene = synthetic.make_batch(1000, 1, 25600)[0].numpy().astype(np.float64)
    Tinv = np.linalg.inv(ingest.table_frame_transform())
    return scene[:, :3] @ Tinv[:3, :3].T + Tinv[:3, 3], np.rint(scene[:, 3:6] * 255.0) / 255.0


def _calibrated(frame, **kw):
    """Networks calibrated on the frame's own cropped cloud (the recipe of tests/test_gpu_table_plane.py) -> (score_net,
    region_net, frame, the detector keywords every run of that frame takes)."""
    from regnet_for_3d_grasping_amd import detect, np_random, pipeline, synthetic
    from regnet_for_3d_grasping_amd.get_regiondataset import get_grasp_allobj
    xyz, rgb = frame
    score_net, region_net = pipeline.build_models(DEV)
    score_net.eval()
    region_net.eval()
    probe = detect.GraspDetector(score_net, region_net, **kw)
    np.random.seed(SEED)
    with np_random.deferred(), torch.no_grad():
        pc = probe.ingest((xyz, rgb)).pc.clone()
    synthetic.calibrate_score_head(score_net, pc)
    with torch.no_grad():
        feat, score, _ = score_net(pc)
    np.random.seed(41)
    got = get_grasp_allobj(pc, score, detect.TEST_PARAMS, [], True)
    np.random.seed(5)
    synthetic.calibrate_region_head(region_net, lambda: _region(region_net, got, pc, feat, detect.GRIPPER_PARAMS))
    return score_net, region_net, (xyz, rgb), kw


@pytest.fixture(scope="module")
def detector_parts():
    return _calibrated(_frame())


@pytest.fixture(scope="module")
def scene_parts():
    return _calibrated(_scene_frame(), bounds=SCENE_BOUNDS)


def _run(parts, **kw):
    from regnet_for_3d_grasping_amd import detect
    score_net, region_net, frame, base = parts
    detector = detect.GraspDetector(score_net, region_net, **base, **kw)
    np.random.seed(SEED)
    out = detector.detect(frame)
    return detector, out, np.random.get_state()


def _same_state(a, b):
    return a[0] == b[0] and np.array_equal(a[1], b[1]) and a[2:] == b[2:]


@pytest.fixture(scope="module")
def plain(detector_parts):
    return _run(detector_parts)


def test_three_boxes_are_three_objects_and_every_key_equals_the_restatement(detector_parts, plain):
    from regnet_for_3d_grasping_amd import detect
    _, out, state = _run(detector_parts, segment={})
    assert tuple(out) == detect.RESULT_KEYS + detect.SEGMENT_KEYS
    _, want, want_state = plain
    for key in detect.RESULT_KEYS:                              # the rest of the record and numpy's generator: untouched
        assert out[key].dtype == want[key].dtype and out[key].tobytes() == want[key].tobytes(), key
    assert _same_state(state, want_state)
    points32 = out["points"].astype(np.float32)
    mask = ref.above_table_mask(points32, detect.TABLE_HEIGHT, 0.01)
    seg = ref.cluster_points(points32, mask, tolerance=0.01, min_points=50, max_objects=64)
    print("points %d, above the table %d, objects %s, sizes %s" % (len(points32), mask.sum(), seg["num"], seg["size"][:4]))
    assert seg["num"].tolist() == [3, 3]
    assert out["point_object"].dtype == np.int32 and np.array_equal(out["point_object"], seg["label"])
    assert out["object_size"].dtype == np.int32 and np.array_equal(out["object_size"], seg["size"][:3])
    assert out["object_bbox"].dtype == np.float32 and out["object_bbox"].tobytes() == seg["bbox"][:3].tobytes()
    for box in out["object_bbox"]:                              # every object is one of the three box tops
        centre = (box[:3] + box[3:]) / 2
        assert any(abs(centre[0] - cx) < 0.01 and abs(centre[1] - cy) < 0.01 and abs(centre[2] - 0.75 - tall) < 0.01
                   for cx, cy, _, tall in BOXES), box
    obj, _ = ref.assign(out["grasp_stage3"][:, :3], points32, seg["label"], 0.03)
    print("grasps %d, on an object %d" % (len(obj), (obj >= 0).sum()))
    assert out["grasp_object"].dtype == np.int32 and np.array_equal(out["grasp_object"], obj)
    # another source set, other parameters
    _, other, _ = _run(detector_parts, segment={"source": "grasp_stage2", "min_points": 2000, "assign_radius": 0.05})
    seg2 = ref.cluster_points(points32, mask, tolerance=0.01, min_points=2000, max_objects=64)
    assert np.array_equal(other["point_object"], seg2["label"]) and len(other["object_size"]) == seg2["num"][0] < 3
    obj2, _ = ref.assign(other["grasp_stage2"][:, :3], points32, seg2["label"], 0.05)
    assert np.array_equal(other["grasp_object"], obj2)


def _reference_selection(out, source, k, **nms):
    """The restatement's per-object selection of the record's own source set: the rows pose NMS keeps (the device kernel, pinned
    by tests/test_gpu_grasp_nms.py, with the thresholds the detector should have handed on), cut per object in numpy."""
    from regnet_for_3d_grasping_amd import grasp_select
    keep, count = grasp_select.pose_nms_device(torch.from_numpy(out[source]).to(DEV), **nms)
    kept = keep[:int(count.item())].cpu().numpy()
    index, objects = ref.select_per_object(kept, out["grasp_object"], len(out["object_size"]), k)
    per_object = np.bincount(out["grasp_object"][kept][out["grasp_object"][kept] >= 0], minlength=1)
    return index, objects, kept, per_object


def test_grasps_get_their_objects_on_a_frame_where_grasps_survive(scene_parts):
    from regnet_for_3d_grasping_amd import detect
    _, out, _ = _run(scene_parts, segment={})
    assert tuple(out) == detect.RESULT_KEYS + detect.SEGMENT_KEYS
    points32 = out["points"].astype(np.float32)
    mask = ref.above_table_mask(points32, detect.TABLE_HEIGHT, 0.01)
    seg = ref.cluster_points(points32, mask, tolerance=0.01, min_points=50, max_objects=64)
    assert seg["num"][0] >= 2 and np.array_equal(out["point_object"], seg["label"])
    assert np.array_equal(out["object_size"], seg["size"][:seg["num"][0]])
    assert out["object_bbox"].tobytes() == seg["bbox"][:seg["num"][0]].tobytes()
    for source, radius in (("grasp_stage3", 0.03), ("grasp_stage2", 0.02)):
        kw = {} if source == "grasp_stage3" else {"source": source, "assign_radius": radius}
        record = out if not kw else _run(scene_parts, segment=kw)[1]
        obj, _ = ref.assign(record[source][:, :3], points32, seg["label"], radius)
        print("%s: %d grasps, objects %s" % (source, len(obj), np.bincount(obj[obj >= 0], minlength=1).tolist()))
        assert len(record[source]) > 0 and (obj >= 0).any()                       # the comparison below is not one of empty sets
        assert record["grasp_object"].dtype == np.int32 and np.array_equal(record["grasp_object"], obj)


def test_top_k_per_object_selects_at_most_k_of_every_object(scene_parts):
    from regnet_for_3d_grasping_amd import detect
    # thresholds under which nearly every grasp is a distinct one, so that objects hold more than k kept grasps
    tight = {"translation_thresh": 0.002, "rotation_thresh_deg": 2.0, "symmetric": False}
    cases = ((None, "grasp_stage3", {}, 2), (None, "grasp_stage3", {}, 1),
             (dict(tight, source="grasp_stage2", top_k=1), "grasp_stage2", tight, 2),
             (dict(tight, source="grasp_stage3", top_k=1), "grasp_stage3", tight, 1))
    cut = 0
    for select, source, nms, k in cases:
        _, out, _ = _run(scene_parts, select=select, segment={"top_k_per_object": k})
        assert tuple(out) == detect.RESULT_KEYS + detect.SEGMENT_SELECT_KEYS + detect.SEGMENT_KEYS
        index, objects = out["grasp_selected_index"], out["grasp_selected_object"]
        assert index.dtype == np.int64 and objects.dtype == np.int32 and len(out["grasp_object"]) == len(out[source]) > 0
        want_index, want_objects, kept, per_object = _reference_selection(out, source, k, **nms)
        print("%s, k = %d, %s: %d grasps, %d distinct, per object %s -> selected %s" % (
            source, k, "select" if select else "defaults", len(out[source]), len(kept), per_object.tolist(), objects.tolist()))
        assert len(index) > 0 and np.array_equal(index, want_index) and np.array_equal(objects, want_objects)
        assert np.bincount(objects).max() <= k                                     # no object has more than k
        assert len(set(index.tolist())) == len(index) and ((index >= 0) & (index < len(out[source]))).all()
        assert np.array_equal(out["grasp_selected"], out[source][index])           # every selected row is a row of the source set
        assert np.array_equal(objects, out["grasp_object"][index]) and (np.diff(objects) >= 0).all()
        cut += int((per_object > k).any())
        if select is not None:                                                     # the per-frame top_k = 1 does not apply
            assert len(index) > 1
    assert cut >= 1                                                                # objects were actually cut down to k


def test_without_segment_the_record_is_the_one_of_a_detector_built_without_the_argument(detector_parts, plain):
    from regnet_for_3d_grasping_amd import detect
    _, want, want_state = plain
    _, out, state = _run(detector_parts, segment=None)
    assert tuple(out) == tuple(want) == detect.RESULT_KEYS
    for key in detect.RESULT_KEYS:
        assert out[key].dtype == want[key].dtype and out[key].tobytes() == want[key].tobytes(), key
    assert _same_state(state, want_state)
    _, selected, _ = _run(detector_parts, select={"top_k": 5}, segment=None)
    assert tuple(selected) == detect.RESULT_KEYS + detect.SELECT_KEYS
    with pytest.raises(TypeError):
        detect.GraspDetector(detector_parts[0], detector_parts[1], segment="yes")
    with pytest.raises(ValueError):
        detect.GraspDetector(detector_parts[0], detector_parts[1], segment={"tolerance": 0.0})


def test_cli_segment_writes_the_extra_keys(detector_parts, plain, tmp_path):
    from regnet_for_3d_grasping_amd import detect
    score_net, region_net = detector_parts[:2]
    none = argparse.Namespace(segment=False, cluster_tolerance=None, min_object_points=None, max_objects=None,
                              top_k_per_object=None)
    assert detect.segment_from_args(none) is None
    assert detect.segment_from_args(argparse.Namespace(**dict(vars(none), segment=True))) == {}
    flags = argparse.Namespace(segment=True, cluster_tolerance=0.012, min_object_points=40, max_objects=5, top_k_per_object=None)
    given = detect.segment_from_args(flags)
    assert given == {"tolerance": 0.012, "min_points": 40, "max_objects": 5}
    assert detect.segment_from_args(argparse.Namespace(**dict(vars(none), max_objects=3))) == {"max_objects": 3}
    # a dataset record is segmented too: its cloud is in the same table frame
    folder = tmp_path / "scene_data"
    folder.mkdir()
    path = str(folder / "frame.p")
    with open(path, "wb") as f:
        pickle.dump({"view_cloud": plain[1]["points"].astype(np.float32),
                     "view_cloud_color": plain[1]["colors"].astype(np.float32)}, f)
    detector = detect.GraspDetector(score_net, region_net, segment=given)
    np.random.seed(SEED)
    printed = io.StringIO()
    with contextlib.redirect_stdout(printed):
        out, saved = detector.detect_file(path)
    lines = printed.getvalue().strip().splitlines()
    assert saved == str(tmp_path / "scene_data_predict" / "frame.p")
    assert len(lines) == 4 and lines[3] == "object num: %d" % len(out["object_size"])
    with open(saved, "rb") as f:
        record = pickle.load(f)
    assert tuple(record) == detect.RESULT_KEYS + detect.SEGMENT_KEYS
    assert len(record["object_size"]) == 3 and len(record["point_object"]) == len(record["points"])
    seg = ref.cluster_points(record["points"], ref.above_table_mask(record["points"], detect.TABLE_HEIGHT, 0.01),
                             tolerance=0.012, min_points=40, max_objects=5)
    assert np.array_equal(record["point_object"], seg["label"])
