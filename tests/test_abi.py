"""CPU-side checks of the drop-in boundary: the C-ABI library loads and exports every symbol
include/regnet_hip.h declares; the Python binding rejects CPU tensors like the reference's
CHECK_CUDA; top-level import paths of the reference resolve to this implementation."""
import ctypes
import os
import re

import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def declared_symbols():
    text = open(os.path.join(REPO, "include", "regnet_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(regnet_[a-z0-9_]+)\s*\(", text)))


def test_library_exports_every_declared_symbol():
    from regnet_for_3d_grasping_amd import _lib
    lib = ctypes.CDLL(_lib.LIB_PATH)
    names = declared_symbols()
    assert len(names) >= 15
    for name in names:
        assert hasattr(lib, name), "libregnet_hip.so does not export %s" % name
        assert name in _lib.SIGNATURES, "binding has no signature for %s" % name
    assert sorted(_lib.SIGNATURES) == names
    assert _lib.lib.regnet_abi_version() >= 1
    assert b"gfx950" in _lib.lib.regnet_build_info()
    assert _lib.lib.regnet_strerror(-1).decode().startswith("shape")


def test_argument_checks_without_gpu():
    from regnet_for_3d_grasping_amd import _lib
    L = _lib.lib
    # validation happens before any launch, so these are safe without a device
    assert L.regnet_fps_f32(None, 0, 0, 0, 1, 10, 0, None, None, None) == -1      # M <= 0
    assert L.regnet_fps_f32(None, 0, 0, 0, 1, 10, 11, None, None, None) == -1     # N < M
    assert L.regnet_fps_f32(None, 0, 0, 0, 0, 10, 5, None, None, None) == 0       # empty batch
    assert L.regnet_fps_f32(None, 0, 0, 0, 1, 10, 5, None, None, None) == -2      # null pointers
    assert L.regnet_three_nn_f32(None, 0, 0, 0, None, 0, 0, 0, 1, 5, 2, None, None, None) == -1
    assert L.regnet_ball_query_f32(None, 0, 0, 0, None, 0, 0, 0, 1, 5, 5, 0.1, 0, None, None, None) == -1
    assert L.regnet_fps_workspace_bytes(4, 25600, 64) == 0                  # short run: register-resident kernel
    assert L.regnet_fps_workspace_bytes(4, 4096, 2048) == 0
    assert L.regnet_fps_workspace_bytes(4, 5120, 1024) == 4 * 5120 * 4         # level-2 shape: the cluster kernel as well
    assert L.regnet_fps_workspace_bytes(4, 25600, 5120) == 4 * 25600 * 4       # long run: the Morton permutation
    assert L.regnet_fps_f32(1, 3 * 25600, 25600, 1, 1, 25600, 5120, 1, None, None) == -2   # ... which must be provided
    # beyond 25 600 points: B x N words (permutation / running distances) + the cooperating workgroups' exchange area
    # ... + the launch's status word (a cooperating workgroup that lost its partner flags it instead of sampling on)
    assert L.regnet_fps_workspace_bytes(4, 51200, 5120) == 4 * 51200 * 4 + 4 * (2 * 4 * 64 * 8 * 4 + 256) + 256
    assert L.regnet_fps_status_offset_bytes(4, 51200, 5120) == 4 * 51200 * 4 + 4 * (2 * 4 * 64 * 8 * 4 + 256)
    assert L.regnet_fps_status_offset_bytes(4, 25600, 5120) == -1          # one workgroup per scene: nothing to lose
    assert L.regnet_fps_status_offset_bytes(4, 51200, 64) == -1            # short run: not the cooperative cluster kernel
    with pytest.raises(RuntimeError):
        _lib.check(-1, "x")


def test_mlp_layer_argument_checks_without_gpu():
    """regnet_mlp_layer_f32 / regnet_mlp_layer_splitk_f32 return before any launch for every argument they reject (and for an
    empty layer), so invented addresses are never read: 0x1000 stands for a 16-byte aligned buffer."""
    from regnet_for_3d_grasping_amd import _lib
    L = _lib.lib
    SHAPE, NULL, UNSUPPORTED = -1, -2, -3
    p = 0x1000

    def layer(A=p, lda=64, Ka=64, W=p, Kpad=64, scale=p, shift=p, C=p, ldc=128, P=128, N=128, relu=1, pool=0):
        return L.regnet_mlp_layer_f32(A, lda, Ka, W, Kpad, scale, shift, C, ldc, P, N, relu, pool, None)

    assert layer(Ka=62) == SHAPE and layer(Ka=2, lda=4) == SHAPE            # Ka % 4
    assert layer(lda=66) == SHAPE                                            # lda % 4
    assert layer(Kpad=72, Ka=64) == SHAPE and layer(Kpad=8, Ka=8) == SHAPE   # Kpad % 16
    assert layer(Ka=68, lda=68) == SHAPE                                     # Ka > Kpad
    assert layer(P=-1) == SHAPE and layer(N=0) == SHAPE and layer(Kpad=0, Ka=0) == SHAPE and layer(Ka=-4) == SHAPE
    assert layer(A=p + 4) == SHAPE and layer(A=p + 8) == SHAPE and layer(W=p + 4) == SHAPE   # 16-byte alignment of A / W
    for pool in (1, 32, 63, 65, 128, -64):
        assert layer(pool=pool) == UNSUPPORTED
    assert layer(P=100, pool=64) == UNSUPPORTED and layer(P=64 * 3 + 1, pool=64) == UNSUPPORTED
    assert layer(P=0) == 0 and layer(P=0, pool=64) == 0 and layer(P=0, A=None, W=None, scale=None, shift=None, C=None) == 0
    for name in ("A", "W", "scale", "shift", "C"):
        assert layer(**{name: None}) == NULL, name
    # order: shape before pooling support before the empty layer before the pointers
    assert layer(Ka=62, pool=32) == SHAPE and layer(P=0, pool=32) == UNSUPPORTED and layer(A=None, W=p + 4) == NULL

    def splitk(A=p, lda=64, Ka=64, W=p, Kpad=64, scale=p, shift=p, C=p, ldc=128, P=128, N=128, relu=1, ksplit=2, ws=p):
        return L.regnet_mlp_layer_splitk_f32(A, lda, Ka, W, Kpad, scale, shift, C, ldc, P, N, relu, ksplit, ws, None)

    assert splitk(Ka=62) == SHAPE and splitk(lda=66) == SHAPE and splitk(Kpad=72) == SHAPE and splitk(Ka=68, lda=68) == SHAPE
    assert splitk(ksplit=0) == SHAPE and splitk(ksplit=5) == UNSUPPORTED     # at most Kpad / 16 slices
    assert splitk(P=0) == 0
    for name in ("A", "W", "scale", "shift", "C", "ws"):
        assert splitk(**{name: None}) == NULL, name
    assert splitk(ksplit=1, ws=None, A=p + 4) == SHAPE                       # one slice needs no workspace
    assert splitk(A=p + 4) == SHAPE and splitk(W=p + 8) == SHAPE and splitk(ws=p + 4) == SHAPE
    assert L.regnet_mlp_splitk_workspace_bytes(70, 130, 33) == 33 * 70 * 132 * 4
    assert L.regnet_mlp_splitk_workspace_bytes(70, 130, 1) == 0


def test_binding_rejects_cpu_tensors_like_check_cuda():
    from regnet_for_3d_grasping_amd import dgcnn_ext, pn2_ext, region_ops
    x = torch.zeros(1, 3, 8)
    idx = torch.zeros(1, 4, 2, dtype=torch.int64)
    for call in (lambda: pn2_ext.farthest_point_sample(x, 2), lambda: pn2_ext.ball_query(x, x, 0.1, 2),
                 lambda: pn2_ext.point_search(x, x, 3), lambda: pn2_ext.group_points_forward(x, idx),
                 lambda: pn2_ext.group_points_backward(torch.zeros(1, 3, 4, 2), idx, 8),
                 lambda: pn2_ext.interpolate_forward(x, torch.zeros(1, 5, 3, dtype=torch.int64), torch.zeros(1, 5, 3)),
                 lambda: dgcnn_ext.gather_knn_forward(x, idx),
                 lambda: region_ops.radius_candidates(torch.zeros(1, 8, 6), torch.zeros(1, 2, 6), 0.1)):
        with pytest.raises(RuntimeError, match="CUDA tensor"):
            call()


def test_reference_import_paths_resolve_here():
    import importlib
    for name in ("pn2_ext", "dgcnn_ext", "multi_model.utils.pn2_utils.function",
                 "multi_model.utils.pn2_utils.modules", "multi_model.utils.pn2_utils.nn",
                 "multi_model.utils.pointnet2", "multi_model.score_network", "multi_model.gripper_region_network",
                 "dataset_utils.get_regiondataset", "dataset_utils.scoredataset", "dataset_utils.eval_score.eval"):
        mod = importlib.import_module(name)
        assert os.path.abspath(mod.__file__).startswith(REPO), name
    from multi_model.score_network import ScoreNetwork
    from multi_model.utils.pn2_utils import function as _F
    assert ScoreNetwork.__name__ == "ScoreNetwork" and callable(_F.farthest_point_sample)
    from dataset_utils.eval_score.eval import eval_test, eval_validate   # test.py:17
    assert callable(eval_test) and callable(eval_validate)
    for op in ("gather_points", "farthest_point_sample", "ball_query", "group_points", "search_nn_distance",
               "feature_interpolate"):
        assert hasattr(_F, op)
