"""``tsdf.Tracker`` on the device against the restated loop (tests/tsdf_raycast_reference.py ``track``): the rendered sequence of
tests/test_tsdf_raycast_reference_cpu.py.  The model views are bit for bit the restatement's given its volume and pose, the
first registration's correspondences are exact, the poses agree to what the order of the float64 sums leaves, and a frame that
cannot be tracked leaves the volume and the pose as they were."""
import numpy as np
import pytest
import torch

from . import icp_projective_reference as pref
from . import icp_reference as iref
from . import tsdf_raycast_reference as ray
from .test_gpu_tsdf_raycast import _bits, _device_volume, _same
from .test_tsdf_raycast_reference_cpu import (TRACK_FRAMES, TRACK_H, TRACK_K, TRACK_PARAMS, TRACK_VOLUME, TRACK_W, track_sequence)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
f32 = np.float32
# the restated loop's final pose error on this sequence, measured AND asserted by tests/test_tsdf_raycast_reference_cpu.py
# (test_the_loop_tracks_a_rendered_sequence) and recorded in DESIGN.md par. 5 "Raycast and tracking"
from .test_tsdf_raycast_reference_cpu import RESTATED_FINAL_ERROR  # noqa: E402  (held there to the CPU run within 2 %)


def _view(frame):
    xyz, _ = frame
    return (torch.from_numpy(xyz).to(DEV), None, TRACK_W, TRACK_H, TRACK_K)


def _tracker(**params):
    from regnet_for_3d_grasping_amd import tsdf
    return tsdf.Tracker(tsdf.TsdfParams(**TRACK_VOLUME), tsdf.TrackParams(**dict(TRACK_PARAMS, **params)), DEV)


def _floor(cloud, max_dist=0.02, step=1):
    """tests/test_icp_projective_reference_cpu.py ``corner_floor`` for this camera: what float32 leaves of a pose."""
    u = float(np.spacing(f32(np.nanmax(cloud[:, 2])))) / 2
    b = step * float(np.nanmin(cloud[:, 2])) / TRACK_K[0]
    return 8 * (u + max_dist * 4 * u / b)


@pytest.fixture(scope="module")
def sequence():
    poses, frames = track_sequence()
    vol, out = ray.track(frames, TRACK_W, TRACK_H, TRACK_K, TRACK_VOLUME, TRACK_PARAMS, first_pose=poses[0])
    return poses, frames, vol, out


def test_the_sequence_through_the_tracker(sequence):
    from regnet_for_3d_grasping_amd import registration, tsdf
    poses, frames, _, restated = sequence
    tracker = _tracker()
    tracker.reset(poses[0])
    want = ray.Volume(**TRACK_VOLUME)                         # the restated loop's volume, frame by frame
    got = []
    for j, frame in enumerate(frames):
        if j > 0:
            # the device's raycast of the RESTATED volume from the restated pose is the restated model view, bit for bit
            t = tracker.params
            view = _device_volume(want).raycast(restated[j - 1]["pose"], TRACK_K, TRACK_W, TRACK_H, t.near, t.far, t.step, colour=False)
            _same(view, restated[j]["model"], colour=False)
        result = tracker.track(_view(frame))
        got.append(result)
        want.integrate(frame[0], None, TRACK_W, TRACK_H, TRACK_K, restated[j]["pose"])
        if j == 0:
            assert result.status == tsdf.FIRST and result.report is None and result.model is None
            assert np.array_equal(_bits(tracker.volume.D), _bits(want.D)) and np.array_equal(tracker.volume.W.cpu().numpy(), want.W)
            continue
        report, expected = result.report, restated[j]["report"]
        assert result.status == tsdf.TRACKED == restated[j]["status"]
        e_ref, e_gpu = iref.pose_distance(restated[j]["pose"], poses[j]), iref.pose_distance(result.pose, poses[j])
        print("frame %d: device %d iterations, pairs %d, error %.3g; restatement %d iterations, pairs %d, error %.3g; between them %.3g"
              % (j, report["iterations"], report["pairs"], e_gpu, expected["iterations"], expected["pairs"], e_ref,
                 iref.pose_distance(result.pose, restated[j]["pose"])))
        assert e_gpu <= max(2 * e_ref, _floor(frame[0]))
        if j == 1:
            # the same volume and pose on both sides: the same model view, so the registration differs by the order of its sums alone
            _same(result.model, restated[1]["model"], colour=False)
            assert report["status"] == expected["status"] and report["iterations"] == expected["iterations"]
            assert report["history"][:, 0].tolist() == expected["history"][:, 0].tolist()
            # the first step's correspondences, exactly
            icp = tracker.params.icp_params()
            state = torch.from_numpy(registration.initial_state(None, icp)).to(DEV)
            idx = torch.full((TRACK_W * TRACK_H,), -9, dtype=torch.int32, device=DEV)
            registration.step(_view(frame)[0], result.model.target(icp), state, icp, idx_out=idx)
            want_idx, _ = pref.correspond_projective(frame[0], restated[1]["model"]["xyz"], restated[1]["model"]["normals"], TRACK_W,
                                                     TRACK_H, TRACK_K, np.eye(4), icp.max_dist, icp.stride, icp.window)
            assert idx.cpu().numpy().tolist() == want_idx.tolist() and (want_idx >= 0).sum() > 3000
        assert result.hits == int(result.model.counts[2:].sum()) > 0.3 * TRACK_W * TRACK_H
        assert result.counts.dtype == torch.int32 and int(result.counts.sum()) == want.n
    final = iref.pose_distance(got[-1].pose, poses[-1])
    print("final pose error: device %.3g, restatement %.3g (recorded %.3g), holding the first pose %.3g"
          % (final, iref.pose_distance(restated[-1]["pose"], poses[-1]), RESTATED_FINAL_ERROR, iref.pose_distance(poses[0], poses[-1])))
    assert final <= 2 * RESTATED_FINAL_ERROR
    assert tracker.frames == TRACK_FRAMES and tracker.pose.tobytes() == got[-1].pose.tobytes()
    assert int(tracker.volume.W.max()) == TRACK_FRAMES


def test_lost_frames_leave_the_volume_and_the_pose(sequence):
    from regnet_for_3d_grasping_amd import registration, tsdf
    poses, frames, _, _ = sequence
    scene = pref.corner_room(0.5)
    tracker = _tracker()
    tracker.reset(poses[0])
    tracker.track(_view(frames[0]))
    before = tracker.volume.data.clone()
    empty = (np.full((TRACK_W * TRACK_H, 3), np.nan, dtype=np.float32), None)
    jump = np.array(poses[0])
    jump[:3, 3] += poses[0][:3, :3] @ np.array([0.1, 0.0, 0.0])
    jumped = (pref.render(scene, TRACK_W, TRACK_H, TRACK_K, jump), None)
    for frame, status in ((empty, registration.TOO_FEW), (jumped, None)):
        lost = tracker.track(_view(frame))
        assert lost.status == tsdf.LOST and lost.counts is None and lost.pose.tobytes() == poses[0].tobytes()
        assert tracker.pose.tobytes() == poses[0].tobytes() and tracker.frames == 1
        assert torch.equal(tracker.volume.data.view(torch.int32), before.view(torch.int32))
        if status is None:      # the planted 10 cm: the registration finds it, the gate refuses it
            assert lost.report["status"] not in (registration.TOO_FEW, registration.DEGENERATE)
            assert tsdf.relative_motion(lost.report["pose"])[0] > tracker.params.max_translation
        else:
            assert lost.report["status"] == status
    # the other two gates, each alone: the frame that tracks above is refused for its rotation, and for too few hits
    for gate, measured in ((dict(max_rotation=1e-3), lambda r: tsdf.relative_motion(r.report["pose"])[1] > 1e-3),
                           (dict(min_hit_share=0.99), lambda r: r.hits < 0.99 * TRACK_W * TRACK_H),
                           (dict(min_hit_share=0.5), None)):
        other = _tracker(**gate)
        other.reset(poses[0])
        other.track(_view(frames[0]))
        kept = other.volume.data.clone()
        result = other.track(_view(frames[1]))
        if measured is None:                # (and a share the view does reach lets the frame through)
            assert result.status == tsdf.TRACKED and result.hits >= 0.5 * TRACK_W * TRACK_H
            continue
        assert result.status == tsdf.LOST and measured(result) and result.report["status"] == registration.CONVERGED
        assert torch.equal(other.volume.data.view(torch.int32), kept.view(torch.int32)) and other.pose.tobytes() == poses[0].tobytes()
    # a guess near the jumped pose tracks the same frame
    found = tracker.track(_view(jumped), guess=jump @ iref.perturbation(0.2, 2.0))
    assert found.status == tsdf.TRACKED and iref.pose_distance(found.pose, jump) < 2e-3 and tracker.frames == 2
    # a blank wall faced squarely holds three of the six motions: DEGENERATE
    wall = [pref.rectangle((-1, -1, 0.1), (3, 0, 0), (0, 3, 0))]
    pose = np.eye(4)
    pose[:3, :3] = np.diag([1.0, -1.0, -1.0])
    pose[:3, 3] = (0.25, 0.25, 0.6)
    frame = (pref.render(wall, TRACK_W, TRACK_H, TRACK_K, pose), None)
    tracker.reset(pose)
    assert tracker.frames == 0 and int(tracker.volume.W.max()) == 0 and tracker.pose.tobytes() == pose.tobytes()
    assert tracker.track(_view(frame)).status == tsdf.FIRST
    before = tracker.volume.data.clone()
    lost = tracker.track(_view(frame))
    assert lost.status == tsdf.LOST and lost.report["status"] == registration.DEGENERATE and lost.report["pairs"] > 1000
    assert torch.equal(tracker.volume.data.view(torch.int32), before.view(torch.int32)) and tracker.pose.tobytes() == pose.tobytes()


def test_depth_frames_a_side_stream_and_the_parameters(sequence):
    from regnet_for_3d_grasping_amd import depth_frame, tsdf
    poses, frames, _, _ = sequence
    side = torch.cuda.Stream(device=DEV)
    tracker = _tracker(normal_angle=40.0, normal_step=1)
    tracker.reset(poses[0])
    torch.cuda.synchronize()
    for j in range(2):
        depth = np.where(np.isfinite(frames[j][0][:, 2]), frames[j][0][:, 2], 0.0).astype(np.float32).reshape(TRACK_H, TRACK_W)
        result = tracker.track(depth_frame.DepthFrame(depth=depth, intrinsics=TRACK_K), stream=side)
    side.synchronize()
    assert result.status == tsdf.TRACKED and iref.pose_distance(result.pose, poses[1]) < 2e-3
    for bad in (dict(near=0.0), dict(near=1.0, far=0.5), dict(step=-1.0), dict(max_translation=0.0), dict(min_hit_share=1.5),
                dict(iterations=0), dict(window=3)):
        with pytest.raises(ValueError):
            tsdf.TrackParams(**bad)
    assert tsdf.TrackParams.coerce({"far": 2.0}).far == 2.0 and tsdf.TrackParams().icp_params().association == "projective"
    with pytest.raises(TypeError):
        tracker.track("frame")
