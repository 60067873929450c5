"""Expected outputs of tests/test_refpy_crosscheck.py, from the REFERENCE's Python graph (read-only, never copied) over the
CPU oracle, authoring container only:

    python tests/golden/make_golden_refpy.py        # writes tests/golden/s10_refpy_4242.npz

S10  ScoreNet -> region grouping -> grasp-region forward of two 6 144-point scenes drawn from seed 4242 (used by no other
     fixture) with the weights and score-head calibration the test builds (seeded state dicts 5 / 6, then
     ``synthetic.calibrate_score_head`` on the product's own ScoreNetwork, loaded into the reference's).  Stored: scores;
     the feature map at every FEATURE_STRIDE-th point, its maximum over ALL points per scene and channel and max |feature|
     (the whole map is 12.6 MB); centre ids; SHA-256 of both group index tensors (int64); one numpy draw after the forward
     (stream position); the stage-2 grasps; the refine stage's class-1 grasps when it runs.

Inputs are regenerated from seeds; the fixture holds expected OUTPUTS only.
"""
import contextlib
import hashlib
import io
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import _ref_shims  # noqa: E402

sys.path.insert(0, _ref_shims.REPO_ROOT)
from regnet_for_3d_grasping_amd import pipeline, synthetic  # noqa: E402

CFG = dict(scene_seed=4242, B=2, N=6144, score_weights_seed=5, region_weights_seed=6, np_seed=77, gripper_num=64,
           grasp_score_threshold=0.5, reg_channel=10, feature_stride=16)
FIXTURE = os.path.join(HERE, "s10_refpy_4242.npz")


def sha(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def build(score_cls, region_cls):
    params, gparams = pipeline.PARAMS, pipeline.GRIPPER_PARAMS
    s = score_cls(training=True)
    s.load_state_dict(synthetic.seeded_state_dict(s, CFG["score_weights_seed"]))
    r = region_cls(training=True, group_num=params[2], gripper_num=CFG["gripper_num"],
                   grasp_score_threshold=CFG["grasp_score_threshold"], radius=gparams[2], reg_channel=CFG["reg_channel"])
    r.load_state_dict(synthetic.seeded_state_dict(r, CFG["region_weights_seed"]))
    return s.eval(), r.eval()


def main():
    sn, grn, grd = _ref_shims.import_reference()
    from oracle.install import oracle_backend
    from regnet_for_3d_grasping_amd.score_network import ScoreNetwork
    params, gparams = pipeline.PARAMS, pipeline.GRIPPER_PARAMS
    pc = synthetic.make_batch(CFG["scene_seed"], CFG["B"], CFG["N"])
    mir_s = ScoreNetwork(training=True)
    mir_s.load_state_dict(synthetic.seeded_state_dict(mir_s, CFG["score_weights_seed"]))
    mir_s.eval()
    with oracle_backend():
        synthetic.calibrate_score_head(mir_s, pc)
    ref_s, ref_r = build(sn.ScoreNetwork, grn.GripperRegionNetwork)
    ref_s.load_state_dict(mir_s.state_dict())        # the calibrated bn_score, as the test does
    np.random.seed(CFG["np_seed"])
    with torch.no_grad(), contextlib.redirect_stdout(io.StringIO()):
        feat, score, _ = ref_s(pc)
        g = grd.get_grasp_allobj(pc, score, params, [])
        res = ref_r(g[3], g[5], g[2], g[4], g[0], g[1], pc, feat, gparams, None, [])
    np_draw = int(np.random.randint(0, 2 ** 31 - 1))
    out = {"cfg_scene_seed": np.int64(CFG["scene_seed"]), "cfg_np_seed": np.int64(CFG["np_seed"]),
           "cfg_feature_stride": np.int64(CFG["feature_stride"]),
           "score": score.numpy(), "feature_sample": feat[:, ::CFG["feature_stride"], :].contiguous().numpy(),
           "feature_max_over_points": feat.max(dim=1)[0].numpy(), "feature_abs_max": np.float32(feat.abs().max()),
           "center_pc_index": g[1].long().numpy(), "pc_group_index_sha256": np.array(sha(g[2].long())),
           "pc_group_more_index_sha256": np.array(sha(g[4].long())), "np_draw_after": np.int64(np_draw),
           "next_grasp": res[0].numpy(), "refine_ran": np.bool_(res[6] is not None)}
    if res[6] is not None:
        out["select_grasp_class"] = res[6].numpy()
    np.savez_compressed(FIXTURE, **out)
    print("positives %d, stage-2 grasps %s, refine %s, %s: %d bytes" % (int((score > 0.5).sum()), tuple(res[0].shape),
                                                                        res[6] is not None, FIXTURE, os.path.getsize(FIXTURE)))


if __name__ == "__main__":
    main()
