"""CPU side of the deterministic mode: the float32 restatement (tests/det_reference.py) pinned to the float64 one where the
order of the additions cannot matter, the new entry points exported and bound, their argument checks (which return before
any launch), and the flag's raise / warn-once contract."""
import ctypes
import warnings

import numpy as np
import pytest
import torch

from tests import det_reference as D
from tests import f64_reference as R

NEW_SYMBOLS = ["regnet_scatter_plan_bytes", "regnet_scatter_plan", "regnet_scatter_segsum_f32",
               "regnet_scatter_max_grad_det_f32", "regnet_bn_det_workspace_bytes", "regnet_bn_relu_train_fwd_det_f32",
               "regnet_bn_relu_train_bwd_det_f32", "regnet_bn_train_stats_det_f32"]


@pytest.fixture
def deterministic():
    was, warn = torch.are_deterministic_algorithms_enabled(), torch.is_deterministic_algorithms_warn_only_enabled()
    try:
        yield
    finally:
        torch.use_deterministic_algorithms(was, warn_only=warn)


def _ints(rng, shape):
    return torch.from_numpy(rng.integers(-64, 64, shape).astype(np.float32))


def test_restatement_matches_float64_on_integer_gradients():
    rng = np.random.default_rng(0)
    B, C, N1, N2, K = 2, 3, 17, 9, 5
    idx = torch.from_numpy(rng.integers(-2, N1 + 2, (B, N2, K)))
    g = _ints(rng, (B, C, N2, K))
    assert torch.equal(D.group_points_backward(g, idx, N1).double(), R.group_points_backward(g.double(), idx, N1))
    assert torch.equal(D.gather_knn_backward(g, idx).double(), R.gather_knn_backward(g.double(), idx))
    M, N = 7, 13
    idx3 = torch.from_numpy(rng.integers(-1, M + 1, (B, N, 3)))
    w = torch.from_numpy(rng.integers(-3, 4, (B, N, 3)).astype(np.float32))
    g3 = _ints(rng, (B, C, N))
    assert torch.equal(D.interpolate_backward(g3, idx3, w, M).double(),
                       R.interpolate_backward(g3.double(), idx3, w.double(), M))


def test_restatement_adds_in_ascending_source_order():
    # 1 + 2^-24 + 2^-24 = 1 in float32 when added left to right, 1 + 2^-23 when the two small terms go first
    idx = torch.tensor([[[0, 0, 0]]])
    g = torch.tensor([[[[1.0, 2.0 ** -24, 2.0 ** -24]]]], dtype=torch.float32)
    assert float(D.group_points_backward(g, idx, 1)[0, 0, 0]) == 1.0
    g = torch.tensor([[[[2.0 ** -24, 2.0 ** -24, 1.0]]]], dtype=torch.float32)
    assert float(D.group_points_backward(g, idx, 1)[0, 0, 0]) == 1.0 + 2.0 ** -23


def test_scatter_max_grad_restatement():
    dy = torch.tensor([[1.0, 2.0], [3.0, 4.0], [5.0, 6.0]])
    arg = torch.tensor([[1, 0], [1, -1], [0, 0]])
    grad = D.scatter_max_grad(dy, arg, torch.full((2, 2), 10.0))
    assert grad.tolist() == [[15.0, 18.0], [14.0, 10.0]]


def test_new_symbols_exported_and_bound():
    from regnet_for_3d_grasping_amd import _lib
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name
        assert name in _lib.SIGNATURES, name
    assert _lib.lib.regnet_abi_version() == 2


def test_argument_checks_without_gpu():
    from regnet_for_3d_grasping_amd import _lib
    L = _lib.lib
    # the plan has the float64 scratch layout
    assert L.regnet_scatter_plan_bytes(2, 100, 640) == L.regnet_scatter_f64_workspace_bytes(2, 100, 640)
    assert L.regnet_scatter_plan(None, -1, 4, 4, None, None) == -1
    assert L.regnet_scatter_plan(None, 0, 4, 4, None, None) == 0
    assert L.regnet_scatter_plan(None, 1, 4, 4, None, None) == -2
    assert L.regnet_scatter_plan(None, 70000, 4, 4, None, None) == -3
    assert L.regnet_scatter_plan(None, 1, 1 << 30, 4, None, None) == -3
    seg = L.regnet_scatter_segsum_f32
    assert seg(None, 0, 0, 0, 0, 0, None, 1, 1, 4, 4, None, None, None) == -1      # inner <= 0
    assert seg(None, 0, 0, 0, 0, 3, None, 1, 1, 4, 4, None, None, None) == -1      # num_src not a multiple of inner
    assert seg(None, 0, 0, 0, 0, 2, 1, 1, 1, 4, 4, None, None, None) == -1         # weighted needs inner 3
    assert seg(None, 0, 0, 0, 0, 4, None, 1, 0, 4, 4, None, None, None) == 0       # no channels
    assert seg(None, 0, 0, 0, 0, 4, None, 1, 1, 4, 4, None, None, None) == -2      # no plan
    assert L.regnet_scatter_max_grad_det_f32(None, None, 8193, 1, 1, 0, 1, 1, None, None) == -3
    assert L.regnet_scatter_max_grad_det_f32(None, None, 8192, 1, 1, 0, 1, 1, None, None) == -2
    assert L.regnet_scatter_max_grad_det_f32(None, None, 4, 1, 0, 0, 1, 1, None, None) == -1
    # BatchNorm: the sums, then a slot per channel and 8 192-element chunk of every scene
    assert L.regnet_bn_det_workspace_bytes(2, 3, 8192 * 2 + 1) == 3 * 16 + 3 * 2 * 3 * 16
    assert L.regnet_bn_det_workspace_bytes(0, 3, 10) == 0
    assert L.regnet_bn_relu_train_fwd_det_f32(None, -1, 1, 1, None, None, 1e-5, 0.1, None, None, 1, 0, None, None, None,
                                             None, None, None) == -1
    assert L.regnet_bn_relu_train_fwd_det_f32(None, 1, 1, 1, None, None, 1e-5, 0.1, None, None, 1, 0, None, None, None,
                                             None, None, None) == -2
    assert L.regnet_bn_relu_train_bwd_det_f32(None, None, None, None, 1, 1, 1, None, None, None, None, 1, 0, None, None,
                                             None, None, None) == -2
    assert L.regnet_bn_train_stats_det_f32(None, 1, 1, 1, None, None, 1e-5, 0.1, None, None, None, None, None, None,
                                          None, None) == -2


def test_unsupported_raises_or_warns_once(deterministic):
    from regnet_for_3d_grasping_amd import determinism
    torch.use_deterministic_algorithms(False)
    assert not determinism.enabled()
    torch.use_deterministic_algorithms(True)
    assert determinism.enabled()
    with pytest.raises(RuntimeError, match="some_op does not have a deterministic implementation"):
        determinism.unsupported("some_op", "this shape")
    torch.use_deterministic_algorithms(True, warn_only=True)
    determinism._warned.discard("some_op")
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        determinism.unsupported("some_op")
        determinism.unsupported("some_op")
    assert len([w for w in seen if "some_op" in str(w.message)]) == 1
