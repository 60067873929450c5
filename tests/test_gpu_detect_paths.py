"""``GraspDetector(approach={"space": "volume", "field": True, "paths": ...}, volume=...)`` end to end on the two 160 x 120 views
and the synthetic networks of tests/test_gpu_detect_fused.py, the proposals held fixed as in tests/test_gpu_detect_retreat.py: the
record's path keys are ``approach.check_paths`` run by hand on the detector's own volume, field and transform, and
tests/hand_path_reference.py on that field; their order and shapes; ``min_path`` filters the selection; a record without
``paths`` is unchanged key for key; the CLI flags."""
import numpy as np
import pytest
import torch

from . import approach_volume_reference as av_ref
from . import hand_path_reference as ref
from .test_gpu_detect_edt import APPROACH
from .test_gpu_detect_fused import SEED, _run, parts  # noqa: F401  (the module-scoped fixture)
from .test_gpu_detect_tsdf import VOLUME

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SIGNED = dict(unseen="blocked", field=True, field_signed=True, field_max_distance=0.1, margin=0.004, **APPROACH)
PATHS = {"length": 0.08, "steps": 8, "turn_deg": 20.0}


def _by_hand(detector, grasp, transform):
    """``check_paths`` by hand on the detector's volume and field -> the check and the five record entries it stands for."""
    from regnet_for_3d_grasping_amd import approach, detect
    check = approach.check_paths(detector.tsdf_volume, detector.distance_field, grasp[:, :8], detect.DEPTH, detect.WIDTH, PATHS,
                                 to_volume=np.linalg.inv(np.asarray(transform, dtype=np.float64)))
    pose = detect._rows_to_frame(transform, check.waypoint)
    return check, dict(zip(detect.APPROACH_PATH_KEYS, (check.index, check.free_steps, check.certified_steps(), check.margin, pose)))


def test_the_path_keys_equal_check_paths_by_hand_and_nothing_else_changes(parts):  # noqa: F811
    from regnet_for_3d_grasping_amd import approach, detect
    params = approach.PathApproachParams(paths=PATHS, **SIGNED)
    assert approach.ApproachParams.coerce(dict(paths=PATHS, **SIGNED)) == params
    detector = detect.GraspDetector(parts[0], parts[1], volume=VOLUME, approach=dict(paths=PATHS, **SIGNED))
    assert detector.approach == params
    np.random.seed(SEED)
    record = detector.detect(parts[2])
    assert tuple(record) == (detect.RESULT_KEYS + detect.APPROACH_KEYS + detect.APPROACH_VOLUME_KEYS + detect.APPROACH_FIELD_KEYS
                             + detect.APPROACH_SIGNED_KEYS + detect.APPROACH_PATH_KEYS + detect.TSDF_KEYS)
    k = len(record["grasp_stage3"])
    assert k > 0
    transform = detector.transform if detector.table is None else detector.table[0]
    grasp = torch.from_numpy(record[detector.approach_source]).to(DEV)
    _, want = _by_hand(detector, grasp, transform)
    shapes = {"grasp_path_index": ((k,), np.int64), "grasp_path_steps": ((k, 9), np.int32),
              "grasp_path_certified": ((k, 9), np.int32), "grasp_path_margin": ((k,), np.float32),
              "grasp_path_pose": ((k, 12), np.float32)}
    for key, value in want.items():
        value = value.cpu().numpy()
        assert (record[key].shape, record[key].dtype) == shapes[key], key
        assert record[key].tobytes() == np.ascontiguousarray(value).tobytes(), key
    steps, certified, index = record["grasp_path_steps"], record["grasp_path_certified"], record["grasp_path_index"]
    assert ((steps >= 0) & (steps <= 8)).all() and ((index >= 0) & (index < 9)).all() and ((certified >= 0) & (certified <= steps)).all()
    assert (steps[np.arange(k), index] == steps.max(axis=1)).all()            # the pick has the most free steps
    print("%d grasps: free steps of the nine paths %s ..., picked %s" % (k, steps[:4].tolist(), index[:8].tolist()))
    # the record without ``paths`` is what it was, key for key; and the fan beside the paths is the fan alone
    plain, _ = _run(parts, parts[2], volume=VOLUME, approach=approach.ApproachParams(**SIGNED))
    assert tuple(plain) == tuple(key for key in record if key not in detect.APPROACH_PATH_KEYS)
    for key in plain:
        assert plain[key].dtype == record[key].dtype and plain[key].tobytes() == record[key].tobytes(), key


def test_min_path_filters_the_selection_and_the_index_addresses_the_full_set(parts):  # noqa: F811
    """The fixed proposals and the planted slab of tests/test_gpu_detect_retreat.py: six copies of the detector's first grasp along
    the volume's x, three about the voxel that is emptiest in the frame's volume and three in the middle of a planted solid slab.
    A turn about the hand's origin keeps every sample within the hand's own reach of its centre, so that test's distances hold
    for all nine paths: the first three hands are free over the WHOLE of every path, the last three have NO free step on any."""
    from regnet_for_3d_grasping_amd import approach, detect
    select = {"top_k": 50, "translation_thresh": 0.001}
    base = dict(field=True, field_signed=True, paths=PATHS, **APPROACH)       # mode solid: only seen surfaces are obstacles
    detector = detect.GraspDetector(parts[0], parts[1], volume=VOLUME, approach=base, select=select)
    np.random.seed(SEED)
    record = detector.detect(parts[2])
    vol = detector.tsdf_volume
    nx, ny, nz = vol.params.dims
    voxel = float(vol.params.voxel)
    d2 = detector.distance_field.dist2.view(nz, ny, nx)[8:-8, 8:-8, 16:-16]
    best = int(d2.argmax().item())
    assert 25 * 25 <= int(d2.reshape(-1)[best].item()) < 1 << 30
    sz, sy, sx = d2.shape
    ix, iy, iz = best % sx + 16, (best // sx) % sy + 8, best // (sx * sy) + 8
    side = -1 if ix >= nx // 2 else 1
    columns = [ix, ix + side, ix + 2 * side, ix + 26 * side, ix + 27 * side, ix + 28 * side]
    lo, hi = sorted((ix + 17 * side, ix + 37 * side))
    assert 0 <= lo and hi < nx
    vol.D.view(nz, ny, nx)[:, :, lo:hi + 1] = -0.5   # the slab: all y and z
    vol.W.view(nz, ny, nx)[:, :, lo:hi + 1] = 1
    transform = np.asarray(detector.transform if detector.table is None else detector.table[0], dtype=np.float64)
    fixed = np.repeat(record["grasp_stage3"][:1], 6, axis=0)
    for g, column in enumerate(columns):
        centre = np.asarray(vol.origin, dtype=np.float64) + (np.array([column, iy, iz]) + 0.5) * voxel
        fixed[g, :3] = (transform @ np.append(centre, 1.0))[:3]
    fixed = torch.from_numpy(fixed).to(DEV)

    def stage(min_path):
        detector.approach = approach.PathApproachParams(min_path=min_path, **base)
        sets = {"grasp_stage3": fixed}
        keys, extra, _ = detector._select_and_segment(sets, None)
        assert keys == (detect.SELECT_KEYS + detect.APPROACH_KEYS + detect.APPROACH_VOLUME_KEYS + detect.APPROACH_FIELD_KEYS
                        + detect.APPROACH_SIGNED_KEYS + detect.APPROACH_PATH_KEYS)
        return ({key: extra[key].cpu().numpy() for key in detect.APPROACH_PATH_KEYS}, sets["grasp_selected_index"].cpu().numpy(),
                sets["grasp_selected"].cpu().numpy())

    rows, all_six, _ = stage(None)
    print("fixed proposals: free steps %s, certified %s, picked %s, margin %s" % (
        rows["grasp_path_steps"].tolist(), rows["grasp_path_certified"].tolist(), rows["grasp_path_index"].tolist(),
        rows["grasp_path_margin"].tolist()))
    assert sorted(all_six.tolist()) == list(range(6))                         # without the bound nothing is dropped
    assert rows["grasp_path_steps"].tolist() == [[8] * 9] * 3 + [[0] * 9] * 3
    certified = rows["grasp_path_certified"]
    # (a free hand's samples come within 1.4 voxels of the slab at the path's end, less than the slack: the last steps need not be
    # certified.  Up to step 5 of any path they keep 15 - (6.3 + 0.8 * 5 + 0.9) = 3.8 voxels = 3.3 beyond the half-voxel
    # of the signed metres, above the slack's 1.73 and half a step's 0.4 .. 0.55)
    assert (certified[3:] == 0).all() and (certified[:3] >= 5).all() and (certified <= 8).all()
    assert rows["grasp_path_index"][3:].tolist() == [0] * 3                   # all equal: the straight path, listed first
    # the keys of the stage are check_paths by hand on the same set, and the restatement on the detector's own field
    check, want = _by_hand(detector, fixed, transform)
    for key, value in want.items():
        assert rows[key].tobytes() == np.ascontiguousarray(value.cpu().numpy()).tobytes(), key
    field = detector.distance_field
    box = av_ref.gripper_box(detect.DEPTH, detect.WIDTH)
    P = check.P.cpu().numpy()
    want_p, want_r = ref.path_ref(field.dist2.cpu().numpy(), (nx, ny, nz), vol.origin, voxel, int(field.outside), P, box, voxel,
                                  detect.DEPTH, check.thresh, True)
    want_d = ref.disp_ref(P, box)
    picked = ref.pick_ref(want_r)
    assert np.array_equal(rows["grasp_path_steps"], want_r[:, :, 0]) and np.array_equal(rows["grasp_path_index"], picked[:, 0])
    assert np.array_equal(rows["grasp_path_certified"],
                          ref.certified_ref(want_p, want_d, voxel, True, ref.default_slack(voxel, voxel), 0.0))
    assert np.array_equal(rows["grasp_path_margin"], ref.metres_ref(picked[:, 2], voxel, True))
    assert np.isfinite(rows["grasp_path_margin"][:3]).all() and (rows["grasp_path_margin"][:3] > 0).all()
    assert np.isinf(rows["grasp_path_margin"][3:]).all()
    # the pre-grasp pose: the hand's own rotation, its origin 8 cm away for the free hands, unmoved for the others
    pose = rows["grasp_path_pose"].reshape(6, 3, 4)
    centre = fixed[:, :3].cpu().numpy()
    moved = np.linalg.norm(pose[:, :, 3] - centre, axis=1)
    assert np.allclose(moved[:3], 0.08, atol=1e-5) and np.allclose(moved[3:], 0.0, atol=1e-6)
    for g in range(3):                               # (every path moves the hand's origin, the default pivot, by the 8 cm)
        if rows["grasp_path_index"][g] == 0:
            assert np.allclose(pose[g, :, 3], centre[g] - pose[g, :, 0] * 0.08, atol=1e-5)
    assert np.allclose(pose[:, :, :3] @ pose[:, :, :3].transpose(0, 2, 1), np.eye(3), atol=1e-5)
    # the certified length of the free hands is 5 cm or more: a bound under it drops the three hands in the slab, and only them
    sure = ref.length_ref(want_d, picked, rows["grasp_path_certified"][np.arange(6), picked[:, 0]])
    assert np.array_equal(check.certified_length.cpu().numpy(), sure) and (sure[:3] > 0.0499).all() and (sure[3:] == 0).all()
    for bound, kept in ((0.0, [0, 1, 2, 3, 4, 5]), (0.01, [0, 1, 2]), (0.04, [0, 1, 2]), (0.2, [])):
        again, index, selected = stage(bound)
        assert sorted(index.tolist()) == kept, (bound, index)
        assert np.array_equal(selected, fixed.cpu().numpy()[index])           # the index addresses the full set
        for key in rows:
            assert again[key].shape[0] == 6 and again[key].tobytes() == rows[key].tobytes(), key


def test_the_value_errors_and_the_cli_flags(parts):  # noqa: F811
    from regnet_for_3d_grasping_amd import approach, detect
    P = approach.PathApproachParams
    with pytest.raises(ValueError, match="field=True"):
        P(space="volume", paths=True)
    with pytest.raises(ValueError, match='space="volume"'):
        P(paths=True)
    with pytest.raises(ValueError, match="paths=True"):
        P(space="volume", field=True, min_path=0.05)
    with pytest.raises(ValueError, match="min_path must be"):
        P(space="volume", field=True, paths=True, min_path=-0.01)
    with pytest.raises(ValueError, match="field_signed=True"):
        P(space="volume", field=True, paths={"min_margin": -0.001})
    assert P(space="volume", field=True, paths=False) == P(space="volume", field=True) and not P(space="volume", field=True).filters()
    assert P(space="volume", field=True, paths=True).paths == approach.PathParams()
    parser = detect.build_parser()
    required = ["--folder", "x", "--load-score-path", "a", "--load-region-path", "b"]
    args = parser.parse_args(required + ["--tsdf", "--approach-space", "volume", "--approach-paths", "--path-turn", "30",
                                         "--path-length", "0.08", "--path-steps", "8", "--path-pivot", "0.01", "0", "-0.02",
                                         "--min-path", "0.04"])
    given = detect.approach_from_args(args)
    assert given == {"space": "volume", "field": True, "min_path": 0.04,
                     "paths": {"turn_deg": 30.0, "length": 0.08, "steps": 8, "pivot": (0.01, 0.0, -0.02)}}
    built = detect.GraspDetector(parts[0], parts[1], volume=detect.volume_from_args(args), approach=given)
    assert built.approach == P(space="volume", field=True, min_path=0.04,
                               paths=approach.PathParams(turn_deg=30.0, length=0.08, steps=8, pivot=(0.01, 0.0, -0.02)))
    assert built.approach.filters() and built.approach.retreat is None
    assert detect.approach_from_args(parser.parse_args(required + ["--approach-space", "volume", "--approach-paths"])) == {
        "space": "volume", "paths": True, "field": True}
    assert detect.approach_from_args(parser.parse_args(required + ["--approach-space", "volume", "--min-path", "0.02"])) == {
        "space": "volume", "paths": True, "field": True, "min_path": 0.02}
    assert detect.approach_from_args(parser.parse_args(required + ["--approach-space", "volume", "--approach-retreat"])) == {
        "space": "volume", "retreat": True, "field": True}                    # the fan's flags are what they were
    assert detect.APPROACH_PATH_KEYS == ("grasp_path_index", "grasp_path_steps", "grasp_path_certified", "grasp_path_margin",
                                         "grasp_path_pose")
