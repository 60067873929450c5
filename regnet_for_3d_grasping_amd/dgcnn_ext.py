"""``dgcnn_ext`` for MI355X (multi_model/utils/pn2_utils/functions/csrc/main.cpp:3-6).

Used only by EdgeFeatureInterpolator, which no REGNet network instantiates; kept for API
completeness on top of the group_points kernels.  float32 or float64 (see pn2_ext).
"""
import torch

from . import _lib
from .pn2_ext import _entry, _eq, _need_float, _need_i64, _scatter_backward

_call = _lib.call


def gather_knn_forward(input, index):
    """input (B,C,N), index (B,NI,K) -> (B,C,NI,K).  gather_knn_kernel.cu:27-50."""
    _need_float(input, "input")
    _need_i64(index, "index")
    _eq(input.dim(), 3, "input.dim() does not equal to 3")
    _eq(index.dim(), 3, "index.dim() does not equal to 3")
    _eq(index.size(0), input.size(0), "index.size(0) does not equal to batch_size")
    B, C, N = input.shape
    _, NI, K = index.shape
    idx = index.contiguous()
    out = torch.empty((B, C, NI, K), dtype=input.dtype, device=input.device)
    _call(_entry("gather_knn_fwd", input), input, input.data_ptr(), *input.stride(), idx.data_ptr(), B, C, N, NI, K,
          out.data_ptr())
    return out


def gather_knn_backward(grad_output, index):
    """grad_output (B,C,N,K), index (B,N,K) -> (B,C,N).  gather_knn_kernel.cu:100-153.  float64, and float32 in
    deterministic mode: summed in ascending (ni, k) order per destination, run to run bit-identical."""
    _need_float(grad_output, "grad_output")
    _need_i64(index, "index")
    _eq(grad_output.dim(), 4, "grad_output.dim() does not equal to 4")
    _eq(index.dim(), 3, "index.dim() does not equal to 3")
    B, C, N, K = grad_output.shape
    _eq(index.size(0), B, "index.size(0) does not equal to batch_size")
    _eq(index.size(2), K, "index.size(2) does not equal to k")
    NI = index.size(1)
    idx = index.contiguous()
    # grad_output rows follow the index rows (NI); the reference sizes grad_input by N
    return _scatter_backward(
        "gather_knn_backward", grad_output, idx, None, B, C, N, NI * K, K, None,
        lambda grad_in, *ws: _call(
            _entry("gather_knn_bwd", grad_output), grad_output, grad_output.data_ptr(), *grad_output.stride(),
            idx.data_ptr(), B, C, N, NI, K, grad_in.data_ptr(), *ws))
