"""Float64 restatement of one shared-MLP layer (include/regnet_hip.h: regnet_mlp_layer_f32) and the error an fp32 evaluation of
it may have.  No GPU dependency: everything runs on the device of the tensors it is given.

    S = A[:, :Ka] . W[:, :Ka]^T        y = scale * S + shift        optional ReLU        optional max over every 64 rows

Tolerance (derived, nothing is fitted to a kernel's output).  u = 2^-24.  The kernels form every product exactly inside an
fp32 FMA and add the Kpad terms of an element in some order: a tree over Kpad leaves has Kpad - 1 additions, so whatever the
order -- one chain, slabs of 128 added to a second register set, k-slices added by a second kernel -- no product passes more
than Kpad roundings.  n = Kpad + ceil(Kpad / 128) + 1 counts the slab additions once more on top (an over-count that keeps
the bound independent of how the tree is cut), and the standard result |fl(sum) - sum| <= gamma_n sum |terms|,
gamma_n = n u / (1 - n u), gives the first term with T = |A| . |W|^T.  The epilogue ``acc * scale + shift`` is two roundings
(one if fused) of magnitudes |scale S| and |scale S + shift|: at most 2 u (|scale S| + |shift|).

    tol = |scale| gamma_n T + 2 u (|scale S| + |shift|)

ReLU and max are 1-Lipschitz (|max_i a_i - max_i b_i| <= max_i |a_i - b_i|), so ReLU leaves the bound as it is and a pooled
output gets the largest bound of its 64 rows.
"""
import torch

U = 2.0 ** -24
POOL = 64


def ceil_to(x, m):
    return (x + m - 1) // m * m


def gamma(n):
    return n * U / (1.0 - n * U)


def chain_length(Kpad):
    return Kpad + (Kpad + 127) // 128 + 1


def pack_weight(w, Kpad):
    """(N, K) -> the packed operand [ceil128(N)][Kpad], zero padded, float32."""
    N, K = w.shape
    out = torch.zeros(ceil_to(N, 128), Kpad, dtype=torch.float32, device=w.device)
    out[:N, :K] = w
    return out


def reference(A, Ka, W, scale, shift, relu, pool):
    """-> (y, S, T) in float64: y as above ((P, N), or (P / 64, N) when ``pool``), S and T = |A| . |W|^T unpooled (P, N).
    A (P, >= Ka) and W (>= N, >= Ka) are read up to column Ka and W up to row N = len(scale)."""
    N = scale.shape[0]
    a = A[:, :Ka].double()
    w = W[:N, :Ka].double()
    S = a @ w.t()
    T = a.abs() @ w.abs().t()
    y = scale.double() * S + shift.double()
    if relu:
        y = torch.relu(y)
    if pool:
        y = y.view(-1, POOL, N).max(dim=1)[0]
    return y, S, T


def tolerance(S, T, scale, shift, Kpad, pool):
    """The elementwise bound of the module docstring, float64, shaped like ``reference``'s y."""
    s, t = scale.double(), shift.double()
    tol = s.abs() * gamma(chain_length(Kpad)) * T + 2.0 * U * ((s * S).abs() + t.abs())
    if pool:
        tol = tol.view(-1, POOL, tol.shape[1]).max(dim=1)[0]
    return tol
