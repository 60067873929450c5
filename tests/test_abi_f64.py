"""CPU-side checks of the float64 entry points of the C ABI: every _f64 symbol is exported and bound, and the argument
checks run before any launch (-1 shape / -2 null pointer), so they hold without a device."""
import ctypes

import pytest
import torch

F64 = ("regnet_fps_f64", "regnet_fps_f64_workspace_bytes", "regnet_ball_query_f64", "regnet_three_nn_f64",
       "regnet_group_points_fwd_f64", "regnet_group_points_bwd_f64", "regnet_interpolate_fwd_f64",
       "regnet_interpolate_bwd_f64", "regnet_gather_knn_fwd_f64", "regnet_gather_knn_bwd_f64",
       "regnet_scatter_f64_workspace_bytes")


def test_f64_symbols_exported_and_bound():
    from regnet_for_3d_grasping_amd import _lib
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in F64:
        assert hasattr(lib, name), name
        assert name in _lib.SIGNATURES, name
    assert _lib.lib.regnet_abi_version() == 2


def test_f64_argument_checks_without_gpu():
    from regnet_for_3d_grasping_amd import _lib
    L = _lib.lib
    assert L.regnet_fps_f64(None, 0, 0, 0, 1, 10, 0, None, None, None) == -1      # M <= 0
    assert L.regnet_fps_f64(None, 0, 0, 0, 1, 10, 11, None, None, None) == -1     # N < M
    assert L.regnet_fps_f64(None, 0, 0, 0, 0, 10, 5, None, None, None) == 0       # empty batch
    assert L.regnet_fps_f64(None, 0, 0, 0, 1, 10, 5, None, None, None) == -2      # null pointers
    assert L.regnet_fps_f64(1, 30, 10, 1, 1, 10, 5, 1, None, None) == -2          # ... the workspace included
    assert L.regnet_fps_f64_workspace_bytes(4, 25600, 5120) == 4 * 25600 * 8
    assert L.regnet_three_nn_f64(None, 0, 0, 0, None, 0, 0, 0, 1, 5, 2, None, None, None) == -1   # N2 < 3
    assert L.regnet_three_nn_f64(None, 0, 0, 0, None, 0, 0, 0, 1, 5, 3, None, None, None) == -2
    assert L.regnet_ball_query_f64(None, 0, 0, 0, None, 0, 0, 0, 1, 5, 5, 0.1, 0, None, None, None) == -1   # K <= 0
    assert L.regnet_ball_query_f64(None, 0, 0, 0, None, 0, 0, 0, 1, 5, 5, 0.1, 4, None, None, None) == -2
    assert L.regnet_group_points_fwd_f64(None, 0, 0, 0, None, -1, 1, 1, 1, 1, None, None) == -1
    assert L.regnet_group_points_fwd_f64(None, 0, 0, 0, None, 1, 1, 1, 1, 1, None, None) == -2
    assert L.regnet_group_points_bwd_f64(None, 0, 0, 0, 0, None, 1, 1, -1, 1, 1, None, None, None) == -1
    assert L.regnet_group_points_bwd_f64(None, 0, 0, 0, 0, None, 1, 1, 4, 1, 1, None, None, None) == -2
    assert L.regnet_interpolate_fwd_f64(None, 0, 0, 0, None, None, 1, 1, 0, 4, None, None) == -1   # M == 0
    assert L.regnet_interpolate_fwd_f64(None, 0, 0, 0, None, None, 1, 1, 4, 4, None, None) == -2
    assert L.regnet_interpolate_bwd_f64(None, 0, 0, 0, None, None, 1, -1, 4, 4, None, None, None) == -1
    assert L.regnet_interpolate_bwd_f64(None, 0, 0, 0, None, None, 1, 1, 4, 4, None, None, None) == -2
    assert L.regnet_gather_knn_fwd_f64(None, 0, 0, 0, None, 1, 1, 1, 1, 1, None, None) == -2
    assert L.regnet_gather_knn_bwd_f64(None, 0, 0, 0, 0, None, 1, 1, 4, 1, 1, None, None, None) == -2
    # a grad_in buffer but no workspace: refused before any launch
    assert L.regnet_group_points_bwd_f64(1, 0, 0, 0, 0, 1, 1, 1, 4, 1, 1, 1, None, None) == -2
    assert L.regnet_scatter_f64_workspace_bytes(2, 10, 7) == 80 + 96 + 64
    assert L.regnet_scatter_f64_workspace_bytes(0, 10, 7) == 0


def test_binding_rejects_other_dtypes_and_cpu_tensors():
    from regnet_for_3d_grasping_amd import dgcnn_ext, pn2_ext
    x = torch.zeros(1, 3, 8, dtype=torch.float64)
    idx = torch.zeros(1, 4, 2, dtype=torch.int64)
    for call in (lambda: pn2_ext.farthest_point_sample(x, 2), lambda: pn2_ext.ball_query(x, x, 0.1, 2),
                 lambda: pn2_ext.point_search(x, x, 3), lambda: pn2_ext.group_points_forward(x, idx),
                 lambda: pn2_ext.interpolate_forward(x, torch.zeros(1, 5, 3, dtype=torch.int64),
                                                     torch.zeros(1, 5, 3, dtype=torch.float64)),
                 lambda: dgcnn_ext.gather_knn_forward(x, idx)):
        with pytest.raises(RuntimeError, match="CUDA tensor"):
            call()
