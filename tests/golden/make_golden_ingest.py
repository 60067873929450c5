"""AUTHORING-CONTAINER ONLY: generate tests/golden/s10_ingest.npz from the reference's own ``utils.noise_color``
(utils.py:426-431) followed by the literal ``np.random.choice`` of test.py:122-127.

``utils.py`` imports transforms3d, tensorboardX and the reference's network / dataset modules (which need open3d and the CUDA
extensions) at module level; ``noise_color`` touches none of them, so they are replaced by EMPTY stand-in modules while the
file is loaded: any use of one would raise AttributeError instead of silently shaping the fixture.

For the two seeded record clouds of tests/ingest_reference.py (30 000 points: drawn without replacement; 9 000 points: with),
as the float32 arrays of the ``.p`` branch (test.py:109-110) and as the float64 array of the ``real_data`` branch, the
fixture records what the reference computed: the drawn rows, the jittered colour of every (channel, 8-bit level) -- the clouds'
colours are level / 255, and the script asserts that the reference's output is that function of the level -- the SHA-256 of
the bytes of ``torch.Tensor(pc[select])``'s float32 rows, and numpy's generator state afterwards.  The colour multiply's
precision and the draw order are thereby pinned against the reference, not against a restatement.
Run:  python tests/golden/make_golden_ingest.py
"""
import contextlib
import hashlib
import importlib.util
import io
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REFERENCE_ROOT = os.environ.get("REGNET_REFERENCE_ROOT", "/root/reference")
ALL_POINTS_NUM = 25600
STAND_INS = ("transforms3d", "tensorboardX", "open3d", "dataset_utils", "dataset_utils.scoredataset", "dataset_utils.eval_score",
             "dataset_utils.eval_score.eval", "multi_model", "multi_model.score_network", "multi_model.gripper_region_network")


def import_reference_utils():
    saved = {name: sys.modules.get(name) for name in STAND_INS}
    try:
        for name in STAND_INS:
            sys.modules[name] = types.ModuleType(name)
        sys.modules["tensorboardX"].SummaryWriter = None
        sys.modules["dataset_utils.scoredataset"].ScoreDataset = None
        sys.modules["multi_model.score_network"].ScoreNetwork = None
        sys.modules["multi_model.gripper_region_network"].GripperRegionNetwork = None
        sys.modules["dataset_utils.eval_score.eval"].eval_test = None
        sys.modules["dataset_utils.eval_score.eval"].eval_validate = None
        spec = importlib.util.spec_from_file_location("_reference_utils", os.path.join(REFERENCE_ROOT, "utils.py"))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
    finally:
        for name, old in saved.items():
            if old is None:
                sys.modules.pop(name, None)
            else:
                sys.modules[name] = old
    return mod


def main():
    import torch
    sys.path.insert(0, os.path.dirname(HERE))
    import ingest_reference as ir
    utils = import_reference_utils()
    out = {}
    for name, cloud_seed, num_points, seed in ir.FIXTURE_CASES:
        xyz, rgb, level = ir.record_cloud(cloud_seed, num_points)
        for tag, dtype in (("f32", np.float32), ("f64", np.float64)):
            pc = np.c_[xyz.astype(dtype), rgb.astype(dtype)]                     # test.py:109-112
            assert pc.dtype == dtype
            np.random.seed(seed)
            with contextlib.redirect_stdout(io.StringIO()):
                pc = utils.noise_color(pc)                                       # :120
            if len(pc) >= ALL_POINTS_NUM:                                        # :122-127
                select = np.random.choice(len(pc), ALL_POINTS_NUM, replace=False)
            elif len(pc) < ALL_POINTS_NUM:
                select = np.random.choice(len(pc), ALL_POINTS_NUM, replace=True)
            state = np.random.get_state()
            final = torch.Tensor(pc[select]).numpy()                             # :127-129
            assert final.dtype == np.float32 and pc.dtype == dtype
            table = np.zeros((3, 256), dtype=dtype)
            for c in range(3):
                table[c, level[:, c]] = pc[:, 3 + c]
                assert np.array_equal(table[c, level[:, c]], pc[:, 3 + c])      # a function of (channel, level)
                assert len(np.unique(level[:, c])) == 256
            key = "%s_%s_" % (name, tag)
            out[key + "select"] = select.astype(np.uint16)
            assert np.array_equal(out[key + "select"].astype(np.int64), select)
            out[key + "color_table"] = table
            out[key + "pc_sha256"] = np.frombuffer(hashlib.sha256(np.ascontiguousarray(final).tobytes()).digest(), dtype=np.uint8)
            out[key + "state_key"] = np.asarray(state[1], dtype=np.uint32)
            out[key + "state_pos"] = np.int64(state[2])
            print(key, "rows", len(pc), "replace", len(pc) < ALL_POINTS_NUM, "pos", state[2])
    np.savez_compressed(os.path.join(HERE, "s10_ingest.npz"), **out)
    print("numpy", np.__version__, "->", os.path.getsize(os.path.join(HERE, "s10_ingest.npz")), "bytes")


if __name__ == "__main__":
    main()
