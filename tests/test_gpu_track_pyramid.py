"""``tsdf.Tracker`` coarse to fine on the device against the restated loop (tests/depth_pyramid_reference.py ``track_pyramid``):
the rendered sequence of tests/test_tsdf_raycast_reference_cpu.py.  Frame by frame from the restated volume and pose the device
ends every level at the restatement's iteration and status with the restatement's pair counts; running free it stays within
twice the restatement's own error against the rendered poses (the rule of tests/test_gpu_tsdf_track.py); a coarse level that
fails loses the frame and leaves the volume; and with one level and no smoothing the new fields change nothing."""
import numpy as np
import pytest
import torch

from . import depth_pyramid_reference as pyr
from . import icp_reference as iref
from . import tsdf_raycast_reference as ray
from .test_gpu_tsdf_raycast import _same
from .test_gpu_tsdf_track import _floor, _view
from .test_tsdf_raycast_reference_cpu import TRACK_FRAMES, TRACK_H, TRACK_K, TRACK_PARAMS, TRACK_VOLUME, TRACK_W, track_sequence

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LEVELS = 3
SMOOTH = dict(radius=2, sigma_space=1.5, sigma_depth=0.01)


def _tracker(**params):
    from regnet_for_3d_grasping_amd import tsdf
    return tsdf.Tracker(tsdf.TsdfParams(**TRACK_VOLUME), tsdf.TrackParams(**dict(TRACK_PARAMS, **params)), DEV)


def _restated(frames, poses, **params):
    """The restated loop, and its volume as it stood BEFORE each frame."""
    _, out = pyr.track_pyramid(frames, TRACK_W, TRACK_H, TRACK_K, TRACK_VOLUME, dict(TRACK_PARAMS, **params), first_pose=poses[0])
    vol, before = ray.Volume(**TRACK_VOLUME), []
    for frame, o in zip(frames, out):
        before.append((vol.D.copy(), vol.W.copy()))
        if o["status"] != ray.LOST:
            vol.integrate(frame[0], None, TRACK_W, TRACK_H, TRACK_K, o["pose"])
    return out, before


@pytest.fixture(scope="module")
def sequence():
    poses, frames = track_sequence()
    plain, plain_before = _restated(frames, poses, levels=LEVELS)
    smoothed, smoothed_before = _restated(frames[:3], poses, levels=2, smooth=SMOOTH)
    return poses, frames, plain, plain_before, smoothed, smoothed_before


def _frame_by_frame(tracker, frames, poses, restated, before):
    """Every frame registered from the RESTATED volume and pose: both sides see the same model, so they differ by the order of
    the registration's float64 sums alone."""
    from regnet_for_3d_grasping_amd import tsdf
    apart = 0.0
    for j in range(1, len(restated)):
        D, W = before[j]
        tracker.volume.D.copy_(torch.from_numpy(D))
        tracker.volume.W.copy_(torch.from_numpy(W))
        tracker.pose, tracker.frames = restated[j - 1]["pose"].copy(), j
        result = tracker.track(_view(frames[j]))
        want = restated[j]
        assert result.status == want["status"] == tsdf.TRACKED
        assert result.levels.dtype == np.int32 and result.levels.tolist() == want["levels"].tolist()
        assert result.report["status"] == want["report"]["status"] and result.report["iterations"] == want["report"]["iterations"]
        assert result.report["history"][:, 0].tolist() == want["report"]["history"][:, 0].tolist()
        _same(result.model, want["model"], colour=False)                  # level 0's view
        assert result.model.width == TRACK_W and result.hits == int(want["model"]["counts"][2:].sum())
        e_ref, e_gpu = iref.pose_distance(want["pose"], poses[j]), iref.pose_distance(result.pose, poses[j])
        apart = max(apart, iref.pose_distance(result.pose, want["pose"]))
        print("frame %d: levels %s, pairs %s, device error %.3g, restatement %.3g, between them %.3g" % (
            j, result.levels.tolist(), [int(p) for p in result.report["history"][:, 0]], e_gpu, e_ref,
            iref.pose_distance(result.pose, want["pose"])))
        assert e_gpu <= max(2 * e_ref, _floor(frames[j][0]))
    return apart


def test_every_frame_against_the_restated_loop(sequence):
    poses, frames, restated, before, _, _ = sequence
    assert [o["status"] for o in restated] == [ray.FIRST] + [ray.TRACKED] * (TRACK_FRAMES - 1)
    tracker = _tracker(levels=LEVELS)
    tracker.reset(poses[0])
    first = tracker.track(_view(frames[0]))
    assert first.levels is None and first.status == "FIRST"
    apart = _frame_by_frame(tracker, frames, poses, restated, before)
    print("device to restatement, the largest over the frames: %.3g" % apart)


def test_the_sequence_running_free(sequence):
    from regnet_for_3d_grasping_amd import tsdf
    poses, frames, restated, _, _, _ = sequence
    tracker = _tracker(levels=LEVELS)
    tracker.reset(poses[0])
    got = [tracker.track(_view(frame)) for frame in frames]
    assert [r.status for r in got] == [tsdf.FIRST] + [tsdf.TRACKED] * (TRACK_FRAMES - 1)
    for j in range(1, TRACK_FRAMES):
        e_ref, e_gpu = iref.pose_distance(restated[j]["pose"], poses[j]), iref.pose_distance(got[j].pose, poses[j])
        assert got[j].levels.shape == (LEVELS, 2) and (np.diff(got[j].levels[::-1, 0]) >= 1).all()
        assert e_gpu <= max(2 * e_ref, _floor(frames[j][0]))
    final_ref = iref.pose_distance(restated[-1]["pose"], poses[-1])
    final = iref.pose_distance(got[-1].pose, poses[-1])
    print("final pose error: device %.3g, restatement %.3g; device to restatement %.3g; holding the first pose %.3g" % (
        final, final_ref, iref.pose_distance(got[-1].pose, restated[-1]["pose"]), iref.pose_distance(poses[0], poses[-1])))
    assert final <= 2 * final_ref
    assert tracker.frames == TRACK_FRAMES and int(tracker.volume.W.max()) == TRACK_FRAMES


def test_smoothing_on_with_depth_frames_and_a_side_stream(sequence):
    from regnet_for_3d_grasping_amd import depth_frame, tsdf
    poses, frames, _, _, restated, before = sequence
    assert [o["status"] for o in restated] == [ray.FIRST, ray.TRACKED, ray.TRACKED]
    tracker = _tracker(levels=2, smooth=SMOOTH)
    tracker.reset(poses[0])
    tracker.track(_view(frames[0]))
    _frame_by_frame(tracker, frames, poses, restated, before)
    # one level, smoothing alone: the new path with `iterations` as its budget
    _, alone = pyr.track_pyramid(frames[:2], TRACK_W, TRACK_H, TRACK_K, TRACK_VOLUME, dict(TRACK_PARAMS, smooth=SMOOTH), first_pose=poses[0])
    tracker = _tracker(smooth=SMOOTH)
    tracker.reset(poses[0])
    tracker.track(_view(frames[0]))
    result = tracker.track(_view(frames[1]))
    assert result.levels.tolist() == alone[1]["levels"].tolist() and result.report["history"][:, 0].tolist() == alone[1]["report"]["history"][:, 0].tolist()
    # DepthFrames in, on a side stream
    side = torch.cuda.Stream(device=DEV)
    tracker = _tracker(levels=2, smooth=SMOOTH, normal_angle=40.0, normal_step=1)
    tracker.reset(poses[0])
    torch.cuda.synchronize()
    for j in range(2):
        depth = np.where(np.isfinite(frames[j][0][:, 2]), frames[j][0][:, 2], 0.0).astype(np.float32).reshape(TRACK_H, TRACK_W)
        result = tracker.track(depth_frame.DepthFrame(depth=depth, intrinsics=TRACK_K), stream=side)
    side.synchronize()
    assert result.status == tsdf.TRACKED and iref.pose_distance(result.pose, poses[1]) < 2e-3 and result.levels.shape == (2, 2)


def test_a_failed_coarse_level_loses_the_frame(sequence):
    """min_pairs = 1500 is more than the 40 x 30 pixels of level 1: its first step ends TOO_FEW, the hand-over leaves that, the
    steps of level 0 return at once, and the frame is LOST by the existing rule."""
    from regnet_for_3d_grasping_amd import registration, tsdf
    poses, frames, _, _, _, _ = sequence
    _, want = pyr.track_pyramid(frames[:2], TRACK_W, TRACK_H, TRACK_K, TRACK_VOLUME, dict(TRACK_PARAMS, levels=2, min_pairs=1500),
                                first_pose=poses[0])
    assert want[1]["status"] == ray.LOST and want[1]["levels"].tolist() == [[1, iref.TOO_FEW], [1, iref.TOO_FEW]]
    tracker = _tracker(levels=2, min_pairs=1500)
    tracker.reset(poses[0])
    tracker.track(_view(frames[0]))
    kept = tracker.volume.data.clone()
    lost = tracker.track(_view(frames[1]))
    assert lost.status == tsdf.LOST and lost.counts is None and lost.levels.tolist() == want[1]["levels"].tolist()
    assert lost.report["status"] == registration.TOO_FEW and lost.report["iterations"] == 1
    assert lost.report["pairs"] == want[1]["report"]["pairs"] and lost.report["pose"].tobytes() == np.eye(4).tobytes()
    assert torch.equal(tracker.volume.data.view(torch.int32), kept.view(torch.int32))
    assert tracker.pose.tobytes() == poses[0].tobytes() and tracker.frames == 1


def test_one_level_without_smoothing_is_the_tracker_as_it_was(sequence):
    from regnet_for_3d_grasping_amd import tsdf
    poses, frames, _, _, _, _ = sequence
    runs = []
    for params in (dict(), dict(levels=1, smooth=None, level_iterations=None, level_dist_scale=2.0)):
        tracker = _tracker(**params)
        assert not tracker.params.pyramid()
        tracker.reset(poses[0])
        results = [tracker.track(_view(frame)) for frame in frames[:3]]
        assert all(r.levels is None for r in results)
        runs.append(([r.pose.tobytes() for r in results], [r.status for r in results], tracker.volume.data.cpu().numpy().tobytes()))
    assert runs[0] == runs[1] and runs[0][1] == [tsdf.FIRST, tsdf.TRACKED, tsdf.TRACKED]


def test_the_parameters():
    from regnet_for_3d_grasping_amd import depth_frame, tsdf
    t = tsdf.TrackParams(levels=3)
    assert t.budgets() == (10, 5, 4) and t.pyramid() and t.icp_params(2).max_dist == 0.08 and t.icp_params(2).iterations == 4
    assert tsdf.TrackParams(levels=4).budgets() == (10, 5, 4, 4) and tsdf.TrackParams(iterations=7).budgets() == (7,)
    assert tsdf.TrackParams(levels=2, level_iterations=[3, 2]).level_iterations == (3, 2)
    assert tsdf.TrackParams(smooth={"radius": 2}).smooth == depth_frame.SmoothParams(radius=2)
    assert tsdf.TrackParams.coerce({"levels": 2, "level_dist_scale": 1.5}).icp_params(1).max_dist == 0.03
    for bad in (dict(levels=0), dict(levels=5), dict(levels=1.5), dict(levels=2, level_iterations=(3,)), dict(level_iterations=(3, 2)),
                dict(levels=2, level_iterations=(0, 3)), dict(levels=2, level_iterations=(40, 25)), dict(level_dist_scale=0.0),
                dict(level_dist_scale=float("nan")), dict(levels=3, level_dist_scale=1e21), dict(smooth={"radius": 9})):
        with pytest.raises(ValueError):
            tsdf.TrackParams(**bad)
    with pytest.raises(TypeError):
        tsdf.TrackParams(smooth=3)
    tracker = _tracker(levels=4)
    tracker.reset()
    small = (torch.full((4 * 6, 3), 0.5, device=DEV), None, 6, 4, (5.0, 5.0, 2.5, 1.5))
    tracker.track(small)
    with pytest.raises(ValueError, match="levels"):
        tracker.track(small)
