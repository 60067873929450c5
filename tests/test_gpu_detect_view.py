"""``GraspDetector(view=ViewParams(...))`` end to end on the two 160 x 120 views and the synthetic networks of
tests/test_gpu_detect_fused.py and on a tracked frame of tests/test_gpu_detect_track.py: the record's ``VIEW_KEYS``, their shapes
and dtypes; ``view_gain`` is ``Volume.view_gain`` called by hand on the detector's own volume; ``interest="grasps"`` needs the
volume-space approach and equals ``interest_hands`` by hand; a record without ``view`` is unchanged key for key; the CLI flags."""
import numpy as np
import pytest
import torch

from .test_gpu_detect_edt import APPROACH
from .test_gpu_detect_fused import SEED, _run, parts  # noqa: F401  (the module-scoped fixture)
from .test_gpu_detect_track import TRACK, sequence
from .test_gpu_detect_tsdf import VOLUME

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
VIEW = {"width": 40, "height": 30, "azimuths": 6, "elevations": 2, "top_k": 3, "radius": 0.6}
SHAPES = {"view_pose": ((12, 4, 4), np.float64), "view_gain": ((12,), np.int32), "view_rays": ((12, 4), np.int32),
          "view_order": ((3,), np.int32), "view_order_gain": ((3,), np.int32)}


def _by_hand(detector, record, camera, interest=None):
    """``view_gain`` and the pick called directly on the detector's volume with the record's poses -> the host dict."""
    from regnet_for_3d_grasping_amd import view_plan
    params = detector.view
    k = params.scaled_intrinsics(*camera)
    result = detector.tsdf_volume.view_gain(record["view_pose"], k, params.width, params.height, params.near, params.far,
                                            params.step, params.max_unknown, params.margin, interest=interest, status=False)
    return result.to_host(params.top_k, params.min_gain)


def _held(record, host):
    for key, (shape, dtype) in SHAPES.items():
        assert (record[key].shape, record[key].dtype) == (shape, dtype), key
    assert np.array_equal(record["view_gain"], host["gain"]) and np.array_equal(record["view_rays"], host["rays"])
    assert np.array_equal(record["view_order"], host["order"]) and np.array_equal(record["view_order_gain"], host["order_gain"])
    assert (record["view_rays"][:, :3].sum(axis=1) == 40 * 30).all()
    poses = record["view_pose"]
    assert np.allclose(np.linalg.det(poses[:, :3, :3]), 1.0) and np.allclose(poses[:, 3], [0, 0, 0, 1])


def test_the_view_keys_on_two_views_equal_view_gain_by_hand_and_nothing_else_changes(parts):  # noqa: F811
    from regnet_for_3d_grasping_amd import detect, view_plan
    mv = parts[2]
    detector = detect.GraspDetector(parts[0], parts[1], volume=VOLUME, view=VIEW)
    np.random.seed(SEED)
    record = detector.detect(mv)
    assert tuple(record) == detect.RESULT_KEYS + detect.TSDF_KEYS + detect.VIEW_KEYS == tuple(record)
    assert detect.VIEW_KEYS == view_plan.VIEW_KEYS
    first = mv.frames[0]
    camera = (first.intrinsics, first.depth.shape[1], first.depth.shape[0])
    _held(record, _by_hand(detector, record, camera))
    gain, order, order_gain = record["view_gain"], record["view_order"], record["view_order_gain"]
    print("gain %s order %s adds %s" % (gain.tolist(), order.tolist(), order_gain.tolist()))
    assert gain.max() > 0 and order[0] == int(np.argmax(gain)) and order_gain[0] == gain.max()      # two views leave space unseen
    # every pose looks at the orbit's target, from the orbit's radius
    eye, forward = record["view_pose"][:, :3, 3], record["view_pose"][:, :3, 2]
    target = eye + 0.6 * forward
    assert np.allclose(target, target[0], atol=1e-9)
    # the record without ``view`` is what it was, key for key and byte for byte
    plain, _ = _run(parts, mv, volume=VOLUME)
    assert tuple(plain) == tuple(key for key in record if key not in detect.VIEW_KEYS)
    for key in plain:
        assert plain[key].dtype == record[key].dtype and plain[key].tobytes() == record[key].tobytes(), key


def test_interest_grasps_counts_the_analysed_hands_and_needs_the_volume_space_approach(parts):  # noqa: F811
    from regnet_for_3d_grasping_amd import approach, detect, view_plan
    with pytest.raises(ValueError, match="space=\"volume\""):
        detect.GraspDetector(parts[0], parts[1], volume=VOLUME, view=dict(VIEW, interest="grasps"))
    with pytest.raises(ValueError, match="space=\"volume\""):
        detect.GraspDetector(parts[0], parts[1], volume=VOLUME, view=dict(VIEW, interest="grasps"), approach={"standoff": 0.05})
    with pytest.raises(ValueError, match="volume=... or track=..."):
        detect.GraspDetector(parts[0], parts[1], view=VIEW)
    params = approach.ApproachParams(**APPROACH)
    mv = parts[2]
    detector = detect.GraspDetector(parts[0], parts[1], volume=VOLUME, approach=params, view=dict(VIEW, interest="grasps"))
    np.random.seed(SEED)
    record = detector.detect(mv)
    assert tuple(record)[-5:] == detect.VIEW_KEYS
    k = len(record[detector.approach_source])
    assert k > 0
    transform = detector.transform if detector.table is None else detector.table[0]
    grasp = torch.from_numpy(record[detector.approach_source]).to(DEV)
    interest, counts = view_plan.interest_hands(detector.tsdf_volume, grasp[:, :8], detect.DEPTH, detect.WIDTH, params,
                                                to_volume=np.linalg.inv(np.asarray(transform, dtype=np.float64)))
    first = mv.frames[0]
    camera = (first.intrinsics, first.depth.shape[1], first.depth.shape[0])
    _held(record, _by_hand(detector, record, camera, interest))
    everything = _by_hand(detector, record, camera)
    print("%d grasps, %d unseen hand voxels; gain %s of %s" % (k, int(interest.sum()), record["view_gain"].tolist(),
                                                                 everything["gain"].tolist()))
    assert (record["view_gain"] <= everything["gain"]).all() and record["view_gain"].max() <= int(interest.sum())
    assert counts.shape == (k,) and int(counts.sum()) >= int(interest.sum())


def test_a_tracked_frame(parts):  # noqa: F811
    from regnet_for_3d_grasping_amd import detect
    frames, _ = sequence()
    detector = detect.GraspDetector(parts[0], parts[1], track=TRACK, volume=VOLUME, view=VIEW)
    np.random.seed(SEED)
    record = detector.detect(frames[0])
    assert tuple(record) == detect.RESULT_KEYS + detect.TSDF_KEYS + detect.TRACK_KEYS + detect.VIEW_KEYS
    camera = (frames[0].intrinsics, frames[0].depth.shape[1], frames[0].depth.shape[0])
    _held(record, _by_hand(detector, record, camera))
    assert record["view_gain"].max() > 0                      # one view leaves much unseen
    with pytest.raises(ValueError, match="this frame has none"):
        detector.detect(parts[3].cloud())                     # a plain cloud fills no volume


def test_the_cli_flags_reach_view_params(parts):  # noqa: F811
    from regnet_for_3d_grasping_amd import detect, view_plan
    parser = detect.build_parser()
    required = ["--folder", "x", "--load-score-path", "a", "--load-region-path", "b"]
    assert detect.view_from_args(parser.parse_args(required)) is None
    assert detect.view_from_args(parser.parse_args(required + ["--next-view"])) == {}
    args = parser.parse_args(required + ["--tsdf", "--approach-space", "volume", "--view-candidates", "6", "2", "--view-radius", "0.4",
                                         "--view-top-k", "3", "--view-interest", "grasps"])
    given = detect.view_from_args(args)
    assert given == {"azimuths": 6, "elevations": 2, "radius": 0.4, "top_k": 3, "interest": "grasps"}
    built = detect.GraspDetector(parts[0], parts[1], volume=detect.volume_from_args(args), approach=detect.approach_from_args(args),
                                 view=given)
    assert isinstance(built.view, view_plan.ViewParams) and built.view.azimuths == 6 and built.view.interest == "grasps"
    assert built.view.radius == 0.4 and built.view.top_k == 3 and built.view.width == 80
    with pytest.raises(ValueError, match="at most 32"):
        view_plan.ViewParams(azimuths=11, elevations=3)
    poses = view_plan.orbit_poses((0.1, 0.2, 0.5), 0.4, [0, 120, 240], [30, 60])
    assert poses.shape == (6, 4, 4) and poses.dtype == np.float64
    assert np.allclose(poses[:, :3, 3] + 0.4 * poses[:, :3, 2], [0.1, 0.2, 0.5])          # z forward, at the target
    assert (poses[:, 1, 1] > 0).all()                         # y down: the image's top points along up = -y
