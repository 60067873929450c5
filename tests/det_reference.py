"""float32 restatement of the deterministic mode's backwards in numpy (test helper, not a test module).

Under ``torch.use_deterministic_algorithms(True)`` the float32 backwards of group_points / gather_knn / interpolate add,
per destination, the contributions in ascending flattened source position (group / gather_knn: m*K + k; interpolate:
n*3 + k, adding the product g*w rounded to float32), sequentially from +0.0, skipping indices outside the destination
range: ``np.add.at`` on float32 arrays.  ``scatter_max_grad`` adds dy[r][f] to grad[arg[r][f]][f] in ascending r, onto the
value already there (arg < 0: nothing).  Same surface as tests/f64_reference.py, for float32 CPU tensors.
"""
import numpy as np
import torch


def _cpu32(x, name):
    if not isinstance(x, torch.Tensor) or x.is_cuda:
        raise RuntimeError("%s: the float32 reference works on CPU tensors" % name)
    if x.dtype != torch.float32:
        raise RuntimeError("%s must be float32" % name)
    return x.contiguous().numpy()


def _scatter(vals, idx, R):
    """vals (C, L) float32, idx (L,) -> (C, R) float32: np.add.at in ascending source position from +0.0."""
    ok = (idx >= 0) & (idx < R)
    acc = np.zeros((R, vals.shape[0]), dtype=np.float32)
    np.add.at(acc, idx[ok], vals[:, ok].T)
    return acc.T


def group_points_backward(grad_output, index, num_points):
    g = _cpu32(grad_output, "grad_output")
    idx = index.contiguous().numpy()
    B, C, N2, K = g.shape
    if idx.shape != (B, N2, K):
        raise RuntimeError("group_points_backward: shape mismatch")
    out = np.zeros((B, C, int(num_points)), dtype=np.float32)
    for b in range(B):
        out[b] = _scatter(g[b].reshape(C, N2 * K), idx[b].reshape(-1), int(num_points))
    return torch.from_numpy(out)


def interpolate_backward(grad_output, index, weight, num_inst):
    g = _cpu32(grad_output, "grad_output")
    w = _cpu32(weight, "weight")
    idx = index.contiguous().numpy()
    B, C, N = g.shape
    if idx.shape != (B, N, 3) or w.shape != (B, N, 3):
        raise RuntimeError("interpolate_backward: shape mismatch")
    out = np.zeros((B, C, int(num_inst)), dtype=np.float32)
    for b in range(B):
        vals = (g[b][:, :, None] * w[b][None, :, :]).reshape(C, N * 3)     # position n*3 + k, float32 products
        out[b] = _scatter(vals, idx[b].reshape(-1), int(num_inst))
    return torch.from_numpy(out)


def gather_knn_backward(grad_output, index):
    return group_points_backward(grad_output, index, grad_output.size(2))


def scatter_max_grad(dy, arg, grad):
    """grad (rows, F) float32 CPU tensor, updated in place and returned: grad[arg[r][f]][f] += dy[r][f] in ascending r."""
    d = _cpu32(dy, "dy")
    a = arg.contiguous().numpy()
    out = grad.numpy()
    R, F = a.shape
    f = np.broadcast_to(np.arange(F), (R, F))
    ok = a >= 0
    np.add.at(out, (a[ok], f[ok]), d[ok])     # row-major order: ascending r for every destination
    return grad
