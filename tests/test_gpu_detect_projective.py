"""Pose refinement by projective association in front of the merge: the two 160 x 120 views and the wrong pose of
``tests/test_gpu_detect_registered.py``, registered by a lookup in the first view's depth image instead of a grid search.
``fusion.refine_poses(..., frames=)`` against the rendered truth and against the restatement on the same clouds, and the
detector's record.

The parameters are ones for which the restatement ALONE meets every condition asserted here (checked on the host before any
device run).  At this resolution the points lie 1 to 2 cm apart (z / f, f = 115 pixels), so: ``normal_step`` 1 -- one pixel is
already a baseline ten times the 1 mm depth quantum, and two pixels along a slanted face leave few neighbours within any jump;
``normal_jump`` 5 cm -- a pixel's step along a face 60 degrees from the image plane is 2 to 3.5 cm deep, which the 2 cm default
(chosen for 640-wide frames, 3 mm a pixel) would cut as if it were an edge; ``max_dist`` stays 2 cm; ``stride`` 3 does not divide
160; the gate at 30 degrees.  "image" normals do meet the conditions, so "fit" is not needed here."""
import numpy as np
import pytest
import torch

from . import icp_projective_reference as pref
from . import icp_reference as ref
from .test_gpu_detect_fused import FUSE, SEED, parts  # noqa: F401  (the fixture: both networks and the two views)
from .test_gpu_detect_registered import REGISTER as NEAREST

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
REGISTER = {"association": "projective", "max_dist": 0.02, "iterations": 10, "stride": 3, "min_pairs": 100, "window": 1,
            "normal_angle": 30.0, "normals": "image", "normal_step": 1, "normal_jump": 0.05}


@pytest.fixture(scope="module")
def views(parts):  # noqa: F811
    """-> dict: the two clouds, the frames, the true poses, the given (wrong) ones, and ``restated``: the restatement's
    registration of view 1 onto view 0's camera on the same clouds, with its own image normals."""
    from regnet_for_3d_grasping_amd import depth_frame, fusion
    mv = parts[2]
    clouds = [depth_frame.to_cloud(frame, device=DEV) for frame in mv.frames]
    truth = [np.eye(4) if p is None else np.array(p) for p in mv.poses]
    given = [truth[0], ref.perturbation(0.5, 4.0) @ truth[1]]
    host = [xyz.cpu().numpy() for xyz, _ in clouds]
    H, W = (int(v) for v in mv.frames[0].depth.shape)
    K = mv.frames[0].intrinsics.astuple()
    normals = [pref.image_normals(xyz, W, H, REGISTER["normal_step"], REGISTER["normal_jump"]) for xyz in host]
    params = dict(ref.DEFAULTS, **{k: REGISTER[k] for k in ("max_dist", "iterations", "stride", "min_pairs", "window")})
    params["min_cos"] = pref.min_cos(REGISTER["normal_angle"])

    def restate(reference, view, start=None):
        start = np.linalg.inv(given[reference]) @ given[view] if start is None else start
        return pref.icp_projective(host[view], host[reference], normals[reference], W, H, K, start, params, normals[view])

    return {"clouds": clouds, "host": host, "truth": truth, "given": given, "frames": mv.frames, "shape": (W, H, K),
            "multiview": fusion.MultiView(mv.frames, given), "restated": restate(0, 1), "restate": restate}


def test_refine_poses_by_lookup_is_the_restatement_and_no_further_from_the_truth(views):
    from regnet_for_3d_grasping_amd import fusion, registration
    poses, report = fusion.refine_poses(views["clouds"], views["given"], REGISTER, frames=views["frames"])
    assert report.shape == (2, 5) and report.dtype == np.float64 and report[0].tolist() == [-1.0, 0.0, 0.0, 0.0, 0.0]
    assert poses[0].tobytes() == views["truth"][0].tobytes()
    want = views["restated"]
    e_given = ref.pose_distance(views["given"][1], views["truth"][1])
    e_ref = ref.pose_distance(views["given"][0] @ want["pose"], views["truth"][1])
    e_gpu = ref.pose_distance(poses[1], views["truth"][1])
    floor = 8 * float(np.spacing(np.float32(np.nanmax(np.abs(views["host"][1])))))
    near, near_report = fusion.refine_poses(views["clouds"], views["given"], NEAREST)
    print("given pose off by %.3g; projective: %s -> %.3g; restatement: status %d, %d iterations, pairs %d, rms %.3g -> %.3g -> %.3g; "
          "floor %.3g; nearest (%s): %s -> %.3g" % (e_given, report[1].tolist(), e_gpu, want["status"], want["iterations"], want["pairs"],
                                                    want["rms_first"], want["rms_last"], e_ref, floor, NEAREST, near_report[1].tolist(),
                                                    ref.pose_distance(near[1], views["truth"][1])))
    assert int(report[1, 0]) == want["status"] and int(report[1, 0]) in (registration.CONVERGED, registration.MAX_ITER)
    assert int(report[1, 1]) == want["iterations"] and int(report[1, 2]) == want["pairs"] >= REGISTER["min_pairs"]
    assert e_gpu <= max(2 * e_ref, floor)
    assert e_gpu <= e_given                                                  # nearer to the rendered pose than the given one
    assert report[1, 4] < report[1, 3]                                       # the surfaces did come together
    # (width, height, Intrinsics) in place of the frames: the same bytes
    W, H, K = views["shape"]
    again, rep = fusion.refine_poses(views["clouds"], views["given"], REGISTER, frames=[(W, H, K), (W, H, K)])
    assert np.stack(again).tobytes() == np.stack(poses).tobytes() and rep.tobytes() == report.tobytes()


def test_another_reference_a_view_that_is_lost_and_the_refusals(views):
    from regnet_for_3d_grasping_amd import fusion, registration
    swapped, rep = fusion.refine_poses(views["clouds"], views["given"], REGISTER, reference=1, frames=views["frames"])
    want = views["restate"](1, 0)
    assert rep[1].tolist() == [-1.0, 0.0, 0.0, 0.0, 0.0] and swapped[1].tobytes() == views["given"][1].tobytes()
    assert (int(rep[0, 0]), int(rep[0, 1]), int(rep[0, 2])) == (want["status"], want["iterations"], want["pairs"]) and rep[0, 2] > 0
    far = np.array(views["given"][1])
    far[:3, 3] += 5.0
    kept, rep = fusion.refine_poses(views["clouds"], [views["given"][0], far], REGISTER, frames=views["frames"])
    assert int(rep[1, 0]) == registration.TOO_FEW and kept[1].tobytes() == far.tobytes()
    with pytest.raises(ValueError, match="frames"):
        fusion.refine_poses(views["clouds"], views["given"], REGISTER)
    with pytest.raises(ValueError, match="one frame per cloud"):
        fusion.refine_poses(views["clouds"], views["given"], REGISTER, frames=views["frames"][:1])
    with pytest.raises(ValueError, match="organised cloud"):
        fusion.refine_poses(views["clouds"], views["given"], REGISTER, frames=[(80, 120, views["shape"][2])] * 2)
    with pytest.raises(TypeError, match="frames"):
        fusion.refine_poses(views["clouds"], views["given"], REGISTER, frames=[None, None])
    with pytest.raises(ValueError, match="register"):
        fusion.refine_poses(views["clouds"], views["given"], dict(REGISTER, association="nearest"), frames=views["frames"])


def test_fuse_frames_and_the_detector_carry_the_poses_and_the_report(parts, views):  # noqa: F811
    from regnet_for_3d_grasping_amd import detect, fusion
    from .test_gpu_detect_fused import _run
    poses, report = fusion.refine_poses(views["clouds"], views["given"], REGISTER, frames=views["frames"])
    fused = fusion.fuse_frames(views["multiview"], None, FUSE, device=DEV, register=REGISTER)
    plain = fusion.fuse_frames(views["multiview"], None, FUSE, device=DEV)
    assert fused.poses.tobytes() == np.stack(poses).tobytes() and fused.register.tobytes() == report.tobytes()
    assert fused.check()[0] < plain.check()[0]                               # fewer voxels: the doubled surfaces are gone
    got, _ = _run(parts, views["multiview"], fuse=FUSE, register=REGISTER)
    assert tuple(got) == detect.RESULT_KEYS + detect.FUSE_KEYS + detect.REGISTER_KEYS
    assert got["fuse_poses"].dtype == got["fuse_register"].dtype == np.float64
    assert got["fuse_poses"].tobytes() == np.stack(poses).tobytes() and got["fuse_register"].tobytes() == report.tobytes()
    detector = detect.GraspDetector(parts[0], parts[1], register=REGISTER)
    assert detector.register.association == "projective" and detector.register.normal_angle == 30.0
    torch.cuda.synchronize()
