"""``GraspDetector(approach=ApproachParams(space="volume"), volume=...)`` end to end on the two 160 x 120 views and the synthetic
networks of tests/test_gpu_detect_fused.py: the record's approach keys are ``approach.analyse_volume`` run by hand on the
detector's own volume, surface and transform; their order; the untouched default; the ValueErrors; the CLI flags."""
import numpy as np
import pytest
import torch

from .test_gpu_detect_fused import SEED, _run, parts  # noqa: F401  (the module-scoped fixture)
from .test_gpu_detect_tsdf import VOLUME

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
# the sample step is the 12.5 mm voxel of this small volume; friction_deg turns the contact pass on the model's normals on
APPROACH = {"space": "volume", "standoff": 0.05, "friction_deg": 35.0}
OLD_KEYS = {"standoff": 0.05, "friction_deg": 35.0, "normal_radius": 0.03, "normal_max_nn": 20}


def _by_hand(detector, record, params):
    """``analyse_volume`` on what the detector holds after ``detect`` -> the ten record entries."""
    from regnet_for_3d_grasping_amd import approach, detect
    transform = detector.transform if detector.table is None else detector.table[0]
    grasp = torch.from_numpy(record[detector.approach_source]).to(DEV)
    res = approach.analyse_volume(detector.tsdf_volume, grasp[:, :8], detect.DEPTH, detect.WIDTH, params,
                                  to_volume=np.linalg.inv(np.asarray(transform, dtype=np.float64)), surface=detector.fused)
    values = (res.clearance, res.width, res.offset, res.opening, res.contact, res.pregrasp, res.clearance_seen, res.clearance_safe,
              res.unseen_share, res.solid_hand)
    return dict(zip(detect.APPROACH_KEYS + detect.APPROACH_VOLUME_KEYS, (v.cpu().numpy() for v in values))), res


@pytest.mark.parametrize("unseen", ["free", "blocked"])
def test_the_record_equals_analyse_volume_by_hand(parts, unseen):  # noqa: F811
    from regnet_for_3d_grasping_amd import approach, detect
    params = approach.ApproachParams(unseen=unseen, **APPROACH)
    detector = detect.GraspDetector(parts[0], parts[1], volume=VOLUME, approach=params)
    np.random.seed(SEED)
    record = detector.detect(parts[2])
    assert tuple(record) == detect.RESULT_KEYS + detect.APPROACH_KEYS + detect.APPROACH_VOLUME_KEYS + detect.TSDF_KEYS
    k = len(record["grasp_stage3"])
    assert k > 0 and detector.approach_source == "grasp_stage3"
    want, res = _by_hand(detector, record, params)
    for key, value in want.items():
        assert record[key].dtype == value.dtype and record[key].shape == value.shape and record[key].tobytes() == value.tobytes(), key
    assert record["grasp_solid_hand"].dtype == np.int32 and record["grasp_unseen"].dtype == np.float32 and record["grasp_pregrasp"].shape == (k, 3)
    policy = "grasp_clearance_safe" if unseen == "blocked" else "grasp_clearance_seen"
    assert np.array_equal(record["grasp_clearance"], record[policy])
    assert (record["grasp_clearance_safe"] <= record["grasp_clearance_seen"]).all()
    counts = res.counts.cpu().numpy()
    assert (counts[:, 6] > 0).all() and (counts[:, 7] < counts[:, 6]).all()          # the hands are inside the volume
    assert ((record["grasp_unseen"] >= 0) & (record["grasp_unseen"] <= 1)).all()
    assert res.contact_counts is not None                                             # the surface's normals were used
    print("%s: %d grasps, clearance seen %.3f safe %.3f (mean), unseen share %.3f, solid hand %d, contact > 0 in %d"
          % (unseen, k, record["grasp_clearance_seen"].mean(), record["grasp_clearance_safe"].mean(), record["grasp_unseen"].mean(),
             int(record["grasp_solid_hand"].sum()), int((record["grasp_contact"] > 0).sum())))


def test_min_clearance_filters_the_selection_on_the_policys_clearance(parts):  # noqa: F811
    from regnet_for_3d_grasping_amd import approach, detect
    params = approach.ApproachParams(unseen="blocked", min_clearance=0.02, **APPROACH)
    detector = detect.GraspDetector(parts[0], parts[1], volume=VOLUME, approach=params, select={"top_k": 50})
    np.random.seed(SEED)
    record = detector.detect(parts[2])
    assert tuple(record) == (detect.RESULT_KEYS + detect.SELECT_KEYS + detect.APPROACH_KEYS + detect.APPROACH_VOLUME_KEYS
                             + detect.TSDF_KEYS)
    index = record["grasp_selected_index"]
    assert (record["grasp_clearance_safe"][index] >= np.float32(0.02)).all()
    assert np.array_equal(record["grasp_selected"], record["grasp_stage3"][index])


def test_the_default_space_is_the_record_without_the_new_fields(parts):  # noqa: F811
    """``space="cloud"`` (the default) against a detector built from a plain dict of the old keys: byte for byte."""
    from regnet_for_3d_grasping_amd import approach, detect
    old, _ = _run(parts, parts[2], volume=VOLUME, approach=dict(OLD_KEYS))
    new, _ = _run(parts, parts[2], volume=VOLUME, approach=approach.ApproachParams(space="cloud", unseen="blocked", step=0.5, margin=0.1,
                                                                                   **OLD_KEYS))
    assert tuple(old) == tuple(new) == detect.RESULT_KEYS + detect.APPROACH_KEYS + detect.TSDF_KEYS
    for key in old:
        assert old[key].dtype == new[key].dtype and old[key].tobytes() == new[key].tobytes(), key
    assert len(old["grasp_clearance"]) == len(old["grasp_stage3"]) > 0


def test_the_value_errors_and_the_cli(parts):  # noqa: F811
    from regnet_for_3d_grasping_amd import depth_frame, detect
    with pytest.raises(ValueError, match='space="volume"'):                            # neither volume nor track
        detect.GraspDetector(parts[0], parts[1], approach=APPROACH)
    with pytest.raises(ValueError, match="space must be"):
        detect.GraspDetector(parts[0], parts[1], volume=VOLUME, approach={"space": "mesh"})
    detector = detect.GraspDetector(parts[0], parts[1], volume=VOLUME, approach=APPROACH)
    merged = parts[3]
    with pytest.raises(ValueError, match='space="volume"'):                            # a plain pair fills no volume
        np.random.seed(SEED)
        detector.detect(merged.cloud())
    with pytest.raises(ValueError, match='space="volume"'):                            # nor does one DepthFrame without track
        np.random.seed(SEED)
        detector.detect(parts[2].frames[0])
    np.random.seed(SEED)
    assert "grasp_unseen" in detector.detect(parts[2])                                 # and the detector still works after them
    assert isinstance(parts[2].frames[0], depth_frame.DepthFrame)
    detect.GraspDetector(parts[0], parts[1], track={}, approach=APPROACH)              # track alone brings a volume
    parser = detect.build_parser()
    required = ["--folder", "x", "--load-score-path", "a", "--load-region-path", "b"]
    args = parser.parse_args(required + ["--tsdf", "--approach-space", "volume", "--approach-unseen", "blocked", "--approach-step",
                                         "0.004", "--approach-margin", "0.002"])
    built = detect.GraspDetector(parts[0], parts[1], volume=detect.volume_from_args(args), approach=detect.approach_from_args(args))
    assert (built.approach.space, built.approach.unseen, built.approach.step, built.approach.margin) == ("volume", "blocked", 0.004, 0.002)
