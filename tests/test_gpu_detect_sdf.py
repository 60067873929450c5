"""``GraspDetector(approach=ApproachParams(space="volume", field=True, field_signed=True, field_max_distance=...), volume=...)``
end to end on the two 160 x 120 views and the synthetic networks of tests/test_gpu_detect_fused.py: the detector builds a signed,
capped field, the record's margin keys and ``grasp_colliding`` are ``approach.analyse_volume(field=...)`` run by hand on the
detector's own volume; a solid planted where fixed proposals' hands are makes ``grasp_margin_hand`` negative and
``grasp_colliding`` non-zero through the detector's own stage, and ``min_margin`` -- negative too, a tolerated penetration --
drops the deeper ones; a record without the new options has exactly the old keys; the ValueErrors; the two CLI flags."""
import numpy as np
import pytest
import torch

from .test_gpu_detect_edt import APPROACH, _by_hand
from .test_gpu_detect_fused import SEED, _run, parts  # noqa: F401  (the module-scoped fixture)
from .test_gpu_detect_tsdf import VOLUME

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def test_the_signed_keys_equal_analyse_volume_by_hand(parts):  # noqa: F811
    from regnet_for_3d_grasping_amd import approach, detect
    cap_m = 0.1
    params = approach.ApproachParams(unseen="blocked", field=True, field_signed=True, field_max_distance=cap_m, margin=0.004,
                                     **APPROACH)
    detector = detect.GraspDetector(parts[0], parts[1], volume=VOLUME, approach=params)
    np.random.seed(SEED)
    record = detector.detect(parts[2])
    assert detect.APPROACH_SIGNED_KEYS == ("grasp_colliding",)
    assert tuple(record) == (detect.RESULT_KEYS + detect.APPROACH_KEYS + detect.APPROACH_VOLUME_KEYS + detect.APPROACH_FIELD_KEYS
                             + detect.APPROACH_SIGNED_KEYS + detect.TSDF_KEYS)
    k = len(record["grasp_stage3"])
    assert k > 0
    built = detector.distance_field
    voxel = float(detector.tsdf_volume.params.voxel)
    assert built.signed and built.cap == int(np.ceil(cap_m / voxel)) and built.mode == "solid_or_unseen" and built.outside
    field = detector.tsdf_volume.distance_field("solid_or_unseen", outside=True, margin=0.004, signed=True, max_distance=cap_m)
    assert torch.equal(field.dist2, built.dist2) and int((built.dist2 == 0).sum()) == 0 and int((built.dist2 < 0).sum()) > 0
    assert int(built.dist2.abs().max()) <= built.cap ** 2
    res = _by_hand(detector, record, params, field)
    for key, value in zip(detect.APPROACH_FIELD_KEYS, (res.margin_hand, res.margin_sweep)):
        value = value.cpu().numpy()
        assert record[key].dtype == np.float32 and record[key].shape == (k,) and record[key].tobytes() == value.tobytes(), key
    colliding = torch.stack([res.colliding_hand, res.colliding_sweep], dim=1).cpu().numpy()
    assert record["grasp_colliding"].dtype == np.int32 and record["grasp_colliding"].shape == (k, 2)
    assert np.array_equal(record["grasp_colliding"], colliding)
    # a negative margin and a colliding sample are the same statement
    assert np.array_equal(record["grasp_margin_hand"] < 0, record["grasp_colliding"][:, 0] > 0)
    assert np.array_equal(record["grasp_margin_sweep"] < 0, record["grasp_colliding"][:, 1] > 0)
    assert (record["grasp_margin_sweep"] <= record["grasp_margin_hand"]).all()
    assert (np.abs(record["grasp_margin_hand"]) <= np.float32(built.cap * voxel)).all()
    print("%d grasps: margin hand %s, colliding %s" % (k, record["grasp_margin_hand"][:6].tolist(),
                                                      record["grasp_colliding"][:6].tolist()))
    # the other keys are what they are without the signed, capped field
    plain, _ = _run(parts, parts[2], volume=VOLUME,
                    approach=approach.ApproachParams(unseen="blocked", field=True, margin=0.004, **APPROACH))
    assert tuple(plain) == (detect.RESULT_KEYS + detect.APPROACH_KEYS + detect.APPROACH_VOLUME_KEYS + detect.APPROACH_FIELD_KEYS
                            + detect.TSDF_KEYS)
    for key in plain:
        if key not in detect.APPROACH_FIELD_KEYS:
            assert plain[key].dtype == record[key].dtype and plain[key].tobytes() == record[key].tobytes(), key


def test_a_planted_solid_makes_the_margin_negative_and_min_margin_drops_the_deeper_grasps(parts):  # noqa: F811
    """The proposals are FIXED as in tests/test_gpu_detect_edt.py: six copies of the detector's first grasp, one voxel apart along
    the volume's x, centred where the frame's volume is emptiest.  They go through the detector's own stage (the signed field of
    the volume as it stands, ``analyse_volume``, the selection) before and after a solid slab is planted over them: all y and
    z, every x from 32 voxels below the first proposal (or the volume's face: in mode ``solid`` the outside is not free space)
    to 9 above it.  A hand sample is within 8 cm = 6.4 voxels of its centre, so every hand lies inside the slab, the free
    voxels above the slab are the nearest to every sample, and a proposal one voxel lower sits one voxel deeper."""
    from regnet_for_3d_grasping_amd import approach, detect
    select = {"top_k": 50, "translation_thresh": 0.001}          # (the copies are 12.5 mm apart: none suppresses another)
    signed = dict(field=True, field_signed=True, **APPROACH)
    detector = detect.GraspDetector(parts[0], parts[1], volume=VOLUME, approach=approach.ApproachParams(**signed), select=select)
    np.random.seed(SEED)
    record = detector.detect(parts[2])
    vol = detector.tsdf_volume
    nx, ny, nz = vol.params.dims
    voxel = float(vol.params.voxel)
    assert detector.distance_field.signed and detector.distance_field.mode == "solid"
    d2 = detector.distance_field.dist2.view(nz, ny, nx)[8:-8, 8:-8, 16:-16]      # away from the faces: the hands stay inside
    best = int(d2.argmax().item())
    assert 25 * 25 <= int(d2.reshape(-1)[best].item()) < 1 << 30
    sz, sy, sx = d2.shape
    ix, iy, iz = best % sx + 16, (best // sx) % sy + 8, best // (sx * sy) + 8
    transform = np.asarray(detector.transform if detector.table is None else detector.table[0], dtype=np.float64)
    fixed = np.repeat(record["grasp_stage3"][:1], 6, axis=0)
    for g in range(6):
        centre = np.asarray(vol.origin, dtype=np.float64) + (np.array([ix - g, iy, iz]) + 0.5) * voxel
        fixed[g, :3] = (transform @ np.append(centre, 1.0))[:3]
    fixed = torch.from_numpy(fixed).to(DEV)

    def stage(min_margin):
        detector.approach = approach.ApproachParams(min_margin=min_margin, **signed)
        sets = {"grasp_stage3": fixed}
        keys, extra, _ = detector._select_and_segment(sets, None)
        assert keys == (detect.SELECT_KEYS + detect.APPROACH_KEYS + detect.APPROACH_VOLUME_KEYS + detect.APPROACH_FIELD_KEYS
                        + detect.APPROACH_SIGNED_KEYS)
        return (extra["grasp_margin_hand"].cpu().numpy(), extra["grasp_colliding"].cpu().numpy(),
                sets["grasp_selected_index"].cpu().numpy())

    before, free, all_six = stage(None)
    assert sorted(all_six.tolist()) == list(range(6)) and (before >= 13 * voxel).all() and (free == 0).all()
    lo = max(ix - 32, 0)
    vol.D.view(nz, ny, nx)[:, :, lo:ix + 10] = -0.5               # the slab over the six hands
    vol.W.view(nz, ny, nx)[:, :, lo:ix + 10] = 1
    after, colliding, _ = stage(None)
    print("planted slab: margin_hand %s, colliding %s" % (after.tolist(), colliding.tolist()))
    assert (after < 0).all() and (colliding[:, 0] > 0).all() and (colliding[:, 1] >= colliding[:, 0]).all()
    assert len(np.unique(after)) > 1 and after.argmax() == 0      # the first proposal is the shallowest
    bound = float(after.max())                                    # a tolerated penetration: only the shallowest pass
    after_again, _, selected = stage(bound)
    assert np.array_equal(after_again, after)
    assert sorted(selected.tolist()) == np.flatnonzero(after >= np.float32(bound)).tolist() and 0 < len(selected) < 6
    assert (before >= np.float32(bound)).all()                    # without the slab none of them would have been dropped


def test_the_value_errors_and_the_two_cli_flags(parts):  # noqa: F811
    from regnet_for_3d_grasping_amd import approach, detect
    with pytest.raises(ValueError, match="field=True"):
        approach.ApproachParams(space="volume", field_signed=True)
    with pytest.raises(ValueError, match="field=True"):
        approach.ApproachParams(space="volume", field_max_distance=0.1)
    with pytest.raises(ValueError, match="field_max_distance"):
        approach.ApproachParams(space="volume", field=True, field_max_distance=0.0)
    fields = [f.name for f in approach.ApproachParams.__dataclass_fields__.values()]
    assert fields[-2:] == ["field_signed", "field_max_distance"]
    parser = detect.build_parser()
    required = ["--folder", "x", "--load-score-path", "a", "--load-region-path", "b"]
    args = parser.parse_args(required + ["--tsdf", "--approach-space", "volume", "--approach-signed", "--approach-field-cap", "0.1"])
    given = detect.approach_from_args(args)
    assert given == {"space": "volume", "field_max_distance": 0.1, "field_signed": True, "field": True}
    built = detect.GraspDetector(parts[0], parts[1], volume=detect.volume_from_args(args), approach=given)
    assert built.approach.field and built.approach.field_signed and built.approach.field_max_distance == 0.1
    assert detect.approach_from_args(parser.parse_args(required + ["--approach-space", "volume", "--approach-signed"])) == {
        "space": "volume", "field_signed": True, "field": True}
    assert detect.approach_from_args(parser.parse_args(required + ["--approach-space", "volume", "--approach-field-cap", "0.05"])) == {
        "space": "volume", "field_max_distance": 0.05, "field": True}
    args = parser.parse_args(required + ["--tsdf", "--approach-space", "volume", "--approach-field"])
    assert detect.approach_from_args(args) == {"space": "volume", "field": True}
    assert detect.approach_from_args(parser.parse_args(required)) is None
