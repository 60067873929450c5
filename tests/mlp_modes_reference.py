"""Float64 restatements of the gather, fused-first-layer and pre-multiplied layers and of the feature-propagation glue kernels
of csrc/mlp.hip (include/regnet_hip.h: regnet_sa_layer1_f32, regnet_sa_layer12_f32, regnet_sa_premul_layer_f32,
regnet_interp_concat_f32, regnet_interp_affine_f32, regnet_score_head_f32), each with the elementwise error an fp32
evaluation may have, and the inputs the tests feed them.  No GPU dependency: everything runs on the device of its tensors.

Every bound is derived the way tests/gemm_reference.py derives its own (u = 2^-24, gamma_n = n u / (1 - n u)); nothing is
fitted to a kernel's output.  Each function returns ``(y, tol, parts)``: the float64 value, the bound (same shape) and the
float64 intermediates the CPU test inspects.

Division.  csrc/build.py passes no flag that pins how an fp32 division is evaluated, so every division is taken at the
documented bound of an fp32 division that is NOT correctly rounded, 2.5 ulp = 5 u relative (``DIV``), not at 0.5 ulp.
"""
import torch

from . import gemm_reference as gref

U = gref.U
DIV = 5.0           # an fp32 division, in units of u (2.5 ulp, see the module docstring)
EXPF = 2.0          # expf: 1 ulp = 2 u
SCALES = (-1.0, 0.5, 1.0, 2.0)


# ---- operands of mlp_gemm_kernel<1 / 3>: bit-determined ---------------------------------------------------------------
def gather_operand(feat, xyz, nbr, ctr, B, M, group, Cf):
    """The fp32 rows [feat[b, nbr] | fl(xyz[nbr] - xyz[ctr])], (B * M * group, Cf + 3); the zero columns up to Kpad are left
    to the caller's Ka.  feat (B, Nsrc, Cf) of any strides or None, xyz (B, 3, Nsrc), nbr (B, M, group), ctr (B, M).  Every
    column is a copy or ONE correctly rounded fp32 subtraction, so float32 torch ops give the kernel's operand bit for bit."""
    assert xyz.dtype == torch.float32 and (feat is None or feat.dtype == torch.float32)
    nb = nbr.reshape(B, M * group, 1)
    pts = xyz.permute(0, 2, 1)
    rel = torch.take_along_dim(pts, nb, 1) - torch.take_along_dim(pts, ctr.reshape(B, M, 1), 1).repeat_interleave(group, 1)
    parts = [rel]
    if Cf:
        parts.insert(0, torch.take_along_dim(feat[:, :, :Cf], nb, 1))
    return torch.cat(parts, 2).reshape(B * M * group, Cf + 3)


def premul_operand(Um, Vm, nbr, B, Nsrc, M, group, C1):
    """The fp32 rows relu(fl(U[b * Nsrc + nbr] - V[p // group])), (B * M * group, C1): one correctly rounded subtraction."""
    assert Um.dtype == torch.float32 and Vm.dtype == torch.float32
    rows = (nbr.reshape(B, M * group) + torch.arange(B, device=nbr.device).view(B, 1) * Nsrc).reshape(-1)
    centre = torch.arange(B * M * group, device=nbr.device) // group
    return torch.relu(Um[rows, :C1] - Vm[centre, :C1])


def layer(A, Ka, w, scale, shift, relu, pool, Kpad):
    """One layer over a bit-determined operand (modes 1 and 3): gemm_reference's value and bound."""
    y, S, T = gref.reference(A, Ka, w, scale, shift, relu, pool)
    return y, gref.tolerance(S, T, scale, shift, Kpad, pool), [S, scale.double() * S, y]


def layer12(x, w1, scale1, shift1, w2, scale, shift, relu, pool, Kpad):
    """Mode 2: x (P, Cf + 3 <= 8) the gathered rows (``gather_operand``), layer 1 (w1 (C1, Cf + 3), scale1, shift1, ReLU)
    evaluated in float64, layer 2 (w2 (N, C1)) in float64 on the UNROUNDED layer-1 values.

    mlp.hip is compiled with contraction on, so the kernel's 8-term VALU dot product is not bit-determined: its layer-1
    value differs from the float64 one by at most D = gemm_reference.tolerance of that layer with K = 8 (a chain of 8
    products, then the affine).  Layer 2 then sums fp32 terms of magnitude <= (|A1| + D) |W|, so T = (|A1| + D) . |W|^T, and
    its exact sum is off by at most D . |W|^T, which the epilogue scales by |scale|:
        tol = |scale| gamma_n T + 2 u (|scale| (|S| + D . |W|^T) + |shift|) + |scale| (D . |W|^T)
    ReLU and max are 1-Lipschitz; a pooled output takes the largest bound of its 64 rows."""
    K1 = x.shape[1]
    A1, S1, T1 = gref.reference(x, K1, w1, scale1, shift1, 1, 0)
    D = gref.tolerance(S1, T1, scale1, shift1, 8, 0)
    N = scale.shape[0]
    w = w2[:N].double()
    S = A1 @ w.t()
    T = (A1.abs() + D) @ w.abs().t()
    prop = D @ w.abs().t()
    y = scale.double() * S + shift.double()
    if relu:
        y = torch.relu(y)
    s = scale.double().abs()
    tol = gref.tolerance(S.abs() + prop, T, scale, shift, Kpad, 0) + s * prop
    if pool:
        y = y.view(-1, gref.POOL, N).max(dim=1)[0]
        tol = tol.view(-1, gref.POOL, N).max(dim=1)[0]
    return y, tol, [S1, scale1.double() * S1, A1, S, scale.double() * S, y]


# ---- 3-NN interpolation ----------------------------------------------------------------------------------------------------
# A weight passes: the division 1 / max(d2, eps) of its own inverse (DIV), the same division inside every term of the
# norm (DIV: the norm's terms are positive, so their relative errors do not add up beyond the largest), the two additions
# of the norm (2) and the division by the norm (DIV).  A term w_k s_k then passes one product and up to two additions (3).
C_WEIGHT = 3 * DIV + 2
C_INTERP = C_WEIGHT + 3            # = 20 roundings per term


def eps32(eps):
    """The fp32 value the entry point receives for ``eps``."""
    return float(torch.tensor(eps, dtype=torch.float32))


def _interp(sparse, idx, dist2, eps):
    """sparse (B, Ns, C) fp32, idx (B, Nd, 3), dist2 (B, Nd, 3) fp32 -> (sum_k w_k s_k, sum_k w_k |s_k|, w) in float64,
    (B * Nd, C): w from the fp32 dist2 values in float64, inv = 1 / max(d2, eps), w = inv / sum inv."""
    B, Nd = idx.shape[:2]
    C = sparse.shape[2]
    inv = 1.0 / torch.clamp(dist2.double(), min=eps32(eps))
    w = inv / inv.sum(2, keepdim=True)
    g = torch.take_along_dim(sparse.double(), idx.reshape(B, Nd * 3, 1), 1).view(B, Nd, 3, C)
    val = (g * w.unsqueeze(-1)).sum(2).reshape(B * Nd, C)
    mag = (g.abs() * w.unsqueeze(-1)).sum(2).reshape(B * Nd, C)
    return val, mag, w


def interp_concat(sparse, idx, dist2, eps, dense, Cout):
    """out[p] = [sum_k w_k sparse[b, idx_k] | dense[b, n] | 0] (P, Cout).  dense (B, Nd, Cd) of any strides or None.
    tol = gamma_20 sum_k w_k |s_k| on the interpolated columns (C_INTERP = 20: two divisions and the norm's division and
    two additions per weight, one product and up to two additions per term); the dense and the pad columns are copies: 0."""
    val, mag, w = _interp(sparse, idx, dist2, eps)
    P, Cs = val.shape
    Cd = 0 if dense is None else dense.shape[2]
    y = torch.zeros(P, Cout, dtype=torch.float64, device=val.device)
    tol = torch.zeros_like(y)
    y[:, :Cs] = val
    tol[:, :Cs] = gref.gamma(C_INTERP) * mag
    if Cd:
        y[:, Cs:Cs + Cd] = dense.reshape(P, Cd).double()
    return y, tol, [w, val]


def interp_affine(ys, idx, dist2, eps, yd, dense_small, wd4, scale, shift, relu):
    """out[p] = act(scale (sum_k w_k Ys[b, idx_k] + Yd[p] + Wd4 . dense_small[p]) + shift).  ys (B, Ns, C), yd (P, >= C) or None,
    dense_small (B, Nd, Cd <= 4) of any strides or None, wd4 (C, 4).

    Roundings: the interpolation as in ``interp_concat`` (20 per term), the four-term skip product (4 products and 3
    additions: at most 4 per term), the addition of Yd (1) and of the skip product (1) -- every part passes at most those
    two -- and the affine epilogue (2, as in gemm_reference):
        dx  = gamma_22 sum_k w_k |Ys_k| + gamma_2 |Yd| + gamma_6 sum_c |Wd4_c| |d_c|
        tol = |scale| dx + 2 u (|scale| (|x| + dx) + |shift|)"""
    val, mag, w = _interp(ys, idx, dist2, eps)
    P, C = val.shape
    x = val.clone()
    dx = gref.gamma(C_INTERP + 2) * mag
    parts = [w, val]
    if yd is not None:
        x = x + yd[:, :C].double()
        dx = dx + gref.gamma(2) * yd[:, :C].double().abs()
    if dense_small is not None:
        d = dense_small.reshape(P, -1).double()
        wq = wd4[:, :d.shape[1]].double()
        q = d @ wq.t()
        parts.append(q)
        x = x + q
        dx = dx + gref.gamma(6) * (d.abs() @ wq.abs().t())
    s, t = scale.double(), shift.double()
    y = s * x + t
    tol = s.abs() * dx + 2.0 * U * (s.abs() * (x.abs() + dx) + t.abs())
    parts += [x, s * x, y]
    if relu:
        y = torch.relu(y)
    return y, tol, parts


def score_head(x, C, w, bias, bn_scale, bn_shift):
    """score[p] = sigmoid(bn_scale (x[p, :C] . w + bias) + bn_shift) -> (score, tol, [v, tol_v]), all (P,).

    v: a lane adds its ceil(C / 64) products (one rounding each for the product if it is not contracted, one per addition),
    the wave adds the 64 lanes in 6 shuffle steps, then the bias: no term passes more than n = ceil(C / 64) + 6 + 2
    roundings, and the affine is two more (as in gemm_reference):
        tol_v = |bn_scale| gamma_n (sum_c |x_c w_c| + |bias|) + 2 u (|bn_scale (S + bias)| + |bn_shift|)
    score = 1 / (1 + expf(-v)): the sigmoid's slope is <= 1/4, expf is off by 1 ulp (2 u, which moves the score by at most
    2 u score (1 - score)), the addition by u and the division by DIV = 5 u:
        tol = tol_v / 4 + 9 u score   (one u of slack for the second-order terms)"""
    xs = x[:, :C].double()
    wv = w.double()
    S = xs @ wv
    T = xs.abs() @ wv.abs()
    n = (C + 63) // 64 + 6 + 2
    v = bn_scale * (S + bias) + bn_shift
    tol_v = abs(bn_scale) * gref.gamma(n) * (T + abs(bias)) + 2.0 * U * ((bn_scale * (S + bias)).abs() + abs(bn_shift))
    score = torch.sigmoid(v)
    return score, tol_v / 4 + (EXPF + 1 + DIV + 1) * U * score, [v, tol_v]


# ---- inputs --------------------------------------------------------------------------------------------------------------
def _gen(device, seed):
    return torch.Generator(device=device).manual_seed(seed)


def _ints(g, lo, hi, shape, device):
    return torch.randint(lo, hi + 1, shape, generator=g, device=device).float()


def _affine(g, n, exact, device):
    if exact:
        scale = torch.tensor(SCALES, device=device)[torch.randint(0, 4, (n,), generator=g, device=device)]
        return scale, _ints(g, -4, 4, (n,), device)
    sign = torch.randint(0, 2, (n,), generator=g, device=device).float() * 2 - 1
    return sign * (torch.rand(n, generator=g, device=device) + 0.5), torch.randn(n, generator=g, device=device) * 0.1


def _values(g, shape, exact, device):
    return _ints(g, -3, 3, shape, device) if exact else torch.randn(shape, generator=g, device=device)


def _weight(g, N, K, exact, device):
    return _ints(g, -2, 2, (N, K), device) if exact else torch.randn(N, K, generator=g, device=device) / K ** 0.5


def _nan_padded(t, pad=4):
    """(rows, C) -> the same values in a (rows, C + pad) buffer whose padding columns hold NaN."""
    out = torch.full((t.shape[0], t.shape[1] + pad), float("nan"), device=t.device)
    out[:, :t.shape[1]] = t
    return out


def sa_indices(c, g, device):
    """nbr (B, M, group) and ctr (B, M) int64 for a row of mlp_modes_cases.SA_CASES."""
    nbr = torch.randint(0, c.Nsrc, (c.B, c.M, c.group), generator=g, device=device)
    ctr = torch.randint(0, c.Nsrc, (c.B, c.M), generator=g, device=device)
    if "extremes" in c.opts:
        # ball-query style: a neighbourhood with `count` members repeats slot 0 behind them
        count = torch.randint(1, c.group + 1, (c.B, c.M, 1), generator=g, device=device)
        slot = torch.arange(c.group, device=device).view(1, 1, c.group)
        nbr = torch.where(slot < count, nbr, nbr[:, :, :1].expand_as(nbr)).contiguous()
        nbr[0, 0], nbr[-1, -1] = 0, c.Nsrc - 1
        nbr[0, 1, ::2], nbr[0, 1, 1::2] = c.Nsrc - 1, 0
        ctr[0, 0], ctr[0, 1], ctr[-1, -1] = 0, c.Nsrc - 1, c.Nsrc - 1
    if "row0_last" in c.opts:
        nbr[0, 0, 0] = c.Nsrc - 1
    return nbr, ctr


def feat_layout(values, layout):
    """values (B, Nsrc, Cf) -> a (B, Nsrc, Cf) VIEW with the same values in the memory layout ``layout``: "clast" contiguous,
    "cfirst" a (B, Cf, Nsrc) buffer, "offset" channels-last starting one float past a 16-byte boundary."""
    B, Ns, Cf = values.shape
    if layout == "cfirst":
        return values.permute(0, 2, 1).contiguous().permute(0, 2, 1)
    if layout == "offset":
        buf = torch.zeros(values.numel() + 4, device=values.device)
        view = buf[1:1 + values.numel()].view(B, Ns, Cf)
        view.copy_(values)
        return view
    assert layout == "clast"
    return values.contiguous()


def sa_inputs(c, exact, seed, device):
    """The tensors of one row of mlp_modes_cases.SA_CASES -> dict.  xyz is a (B, 3, Nsrc) view of a channels-last buffer for
    even B and contiguous for odd B; U and V have ld = C1 + 4 with NaN in the padding columns."""
    g = _gen(device, seed)
    d = {"nbr": None, "ctr": None}
    d["nbr"], d["ctr"] = sa_indices(c, g, device)
    pts = _values(g, (c.B, c.Nsrc, 3), exact, device)
    d["xyz"] = pts.permute(0, 2, 1) if c.B % 2 == 0 else pts.permute(0, 2, 1).contiguous()
    d["feat"] = None
    if c.mode in (1, 2) and c.Cf:
        d["feat"] = feat_layout(_values(g, (c.B, c.Nsrc, c.Cf), exact, device), c.feat)
    if c.mode == 1:
        K = c.Cf + 3
    else:
        K = c.C1
    if c.mode == 2:
        d["w1"] = _weight(g, c.C1, c.Cf + 3, exact, device)
        d["W8"] = torch.zeros(c.C1, 8, device=device)
        d["W8"][:, :c.Cf + 3] = d["w1"]
        d["scale1"], d["shift1"] = _affine(g, c.C1, exact, device)
    if c.mode == 3:
        d["U"] = _nan_padded(_values(g, (c.B * c.Nsrc, c.C1), exact, device))
        d["V"] = _nan_padded(_values(g, (c.B * c.M, c.C1), exact, device) * (1.0 if exact else 0.5))
    d["w"] = _weight(g, c.N, K, exact, device)
    d["scale"], d["shift"] = _affine(g, c.N, exact, device)
    return d


def sa_reference(c, d, relu, Kpad):
    """``(y, tol, parts)`` of a row of SA_CASES on the inputs ``d`` of ``sa_inputs``."""
    if c.mode == 3:
        A = premul_operand(d["U"], d["V"], d["nbr"], c.B, c.Nsrc, c.M, c.group, c.C1)
        return layer(A, c.C1, d["w"], d["scale"], d["shift"], relu, c.pool, Kpad)
    x = gather_operand(d["feat"], d["xyz"], d["nbr"], d["ctr"], c.B, c.M, c.group, c.Cf)
    if c.mode == 1:
        return layer(x, c.Cf + 3, d["w"], d["scale"], d["shift"], relu, c.pool, Kpad)
    return layer12(x, d["w1"], d["scale1"], d["shift1"], d["w"], d["scale"], d["shift"], relu, c.pool, Kpad)


EXACT_EPS = 2.0 ** -10


def interp_indices(B, Nd, Ns, special, exact, g, device):
    """idx (B, Nd, 3) int64, dist2 (B, Nd, 3) fp32 and eps.  float: dist2 = 1e-3 rand, eps = 1e-10.  exact: every triple a
    permutation of (1, 1, 1/2) 2^k, so the weights are 1/4, 1/4, 1/2 exactly; eps = 2^-10.  ``special`` rows, from the last
    row backwards: zero_one -- d2 = 0 in one slot (exact: the other two 2^-9, so the clamped slot is the weight 1/2),
    zero_all -- d2 = 0 in all three (float only: the weights are then 1/3), dup -- j0 = j1 = j2."""
    P = B * Nd
    idx = torch.randint(0, Ns, (P, 3), generator=g, device=device)
    if exact:
        base = torch.tensor([1.0, 1.0, 0.5], device=device)
        perm = torch.argsort(torch.rand(P, 3, generator=g, device=device), dim=1)
        pow2 = torch.tensor([0.125, 0.25, 0.5, 1.0, 2.0, 4.0, 8.0], device=device)
        dist2 = base[perm] * pow2[torch.randint(0, 7, (P, 1), generator=g, device=device)]
        eps = EXACT_EPS
    else:
        dist2 = torch.rand(P, 3, generator=g, device=device) * 1e-3
        eps = 1e-10
    for i, kind in enumerate(special[:P]):
        row = P - 1 - i
        if kind == "dup":
            idx[row] = idx[row, 0]
        elif kind == "zero_one":
            if exact:
                dist2[row] = 2.0 ** -9
            dist2[row, (row + 1) % 3] = 0.0
        elif kind == "zero_all" and not exact:
            dist2[row] = 0.0
    return idx.view(B, Nd, 3), dist2.view(B, Nd, 3), eps


def ic_inputs(c, exact, seed, device):
    g = _gen(device, seed)
    d = {}
    d["idx"], d["dist2"], d["eps"] = interp_indices(c.B, c.Nd, c.Ns, c.special, exact, g, device)
    d["sparse"] = _values(g, (c.B, c.Ns, c.Cs), exact, device)
    d["dense"] = None
    if c.Cd:
        if c.dense == "view":
            d["dense"] = _values(g, (c.B, c.Nd, 3 + c.Cd), exact, device)[:, :, 3:]
        else:
            d["dense"] = _values(g, (c.B, c.Cd, c.Nd), exact, device).permute(0, 2, 1)
    return d


def ia_inputs(c, exact, seed, device):
    """Ys are EVEN integers in the exact mode: the weights 1/4, 1/4, 1/2 and a scale of 1/2 then leave multiples of 1/4."""
    g = _gen(device, seed)
    d = {}
    d["idx"], d["dist2"], d["eps"] = interp_indices(c.B, c.Nd, c.Ns, c.special, exact, g, device)
    d["ys"] = 2.0 * _ints(g, -1, 1, (c.B, c.Ns, c.C), device) if exact else torch.randn(c.B, c.Ns, c.C, generator=g, device=device)
    d["yd"] = _nan_padded(_values(g, (c.B * c.Nd, c.C), exact, device)) if c.yd else None
    d["dense_small"], d["wd4"] = None, None
    if c.Cds:
        d["dense_small"] = _values(g, (c.B, c.Nd, 8), exact, device)[:, :, 3:3 + c.Cds]
        d["wd4"] = torch.zeros(c.C, 4, device=device)
        d["wd4"][:, :c.Cds] = _weight(g, c.C, c.Cds, exact, device)
    d["scale"], d["shift"] = _affine(g, c.C, exact, device)
    return d


SH_BIAS, SH_SCALE, SH_SHIFT, SH_W0 = 0.125, 0.5, 0.25, -0.625
SH_ROWS = {"v_zero": 1.0, "v_plus_100": -320.0, "v_minus_100": 320.0}   # x[row] = (value, 0, 0, ...)


def sh_inputs(c, special, seed, device):
    """x (P, C + 3) with NaN padding, w (C) with w[0] = -0.625, and the scalars bias = 0.125, bn_scale = 0.5, bn_shift = 0.25.
    ``special`` rows (from the last one backwards, never row 0) are zero but for x[row, 0]:  1 gives
    v = 0.5 (1 (-0.625) + 0.125) + 0.25 = 0 in every order of evaluation, -+320 gives v = +-100 + 0.3125."""
    g = _gen(device, seed)
    x = torch.randn(c.P, c.C, generator=g, device=device)
    w = torch.randn(c.C, generator=g, device=device) / c.C ** 0.5
    w[0] = SH_W0
    rows = {}
    for i, kind in enumerate(special[:max(c.P - 1, 0)]):
        row = c.P - 1 - i
        x[row] = 0.0
        x[row, 0] = SH_ROWS[kind]
        rows[kind] = row
    return {"x": _nan_padded(x, 3), "w": w, "rows": rows}
