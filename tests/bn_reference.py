"""Training-mode BatchNorm + ReLU (+ max over the K neighbours) restated in float64 numpy: what csrc/bn_train.hip computes
(regnet_bn_relu_train_fwd_f32 / _bwd_f32, regnet_bn_train_stats_f32), from the reference's modules (conv.py:30-36 BatchNorm +
ReLU, modules.py:245 torch.max over the neighbours) -- no import of the package, no GPU.

  forward   mean and BIASED variance of a channel over (B, L);  z = gamma (x - mean) invstd + beta, invstd = 1 / sqrt(var + eps);
            y = max(z, 0) with ReLU;  with ``group`` = K the maximum over each run of K consecutive elements, the FIRST of several
            equal maxima giving the position; a NaN is a maximum (torch.max; np.argmax takes the first)
            running_mean <- (1 - m) running_mean + m mean,  running_var <- (1 - m) running_var + m var n / (n - 1)
  backward  g = the gradient of y where y > 0 (else 0), with pooling placed on the winning element alone;
            dbeta = sum g, dgamma = sum g xhat, dx = gamma invstd (g - mean(g) - xhat mean(g xhat)),  xhat = (x - mean) invstd

The second half builds float32 inputs whose every DECISION is non-marginal in float64 (``check_margins``): every pre-ReLU value
has |z| >= MARGIN, and in every pool group the two largest values are more than MARGIN apart, or exactly tied because the
input is duplicated.  Two correct float32 implementations then take the same ReLU branch and the same winner everywhere (their
z differ by ~1e-6 of its scale), so a comparison of dx needs no allowance for outliers.  This is a condition on the inputs, not
a tolerance; tests/test_bn_reference_cpu.py asserts it for every case the GPU tests use.
"""
import numpy as np

f32, f64 = np.float32, np.float64
EPS, MOMENTUM = 1e-5, 0.1
MARGIN = 1e-3


# ---- the operation -----------------------------------------------------------------------------------------------------------
def _rows(x):
    """(B, C, ...) -> (B, C, L) float64."""
    x = np.asarray(x)
    return x.astype(f64).reshape(x.shape[0], x.shape[1], -1)


def _per_channel(v):
    return np.asarray(v, dtype=f64)[None, :, None]


def forward(x, gamma, beta, relu=True, group=0, running_mean=None, running_var=None, eps=EPS, momentum=MOMENTUM):
    """-> dict: mean, var (biased), invstd (C,), z (the pre-ReLU values, x's shape), y, index (position of the winner in its
    group, pooled only), running_mean, running_var (None without the old ones).  ``group``: the last axis of a 4-D x."""
    x = np.asarray(x)
    r = _rows(x)
    n = r.shape[0] * r.shape[2]
    mean = r.sum((0, 2)) / n
    with np.errstate(invalid="ignore"):                                # (inf - inf of a poisoned channel: NaN is the answer)
        var = ((r - _per_channel(mean)) ** 2).sum((0, 2)) / n          # two passes: no cancellation
        invstd = 1.0 / np.sqrt(var + eps)
        z = (_per_channel(gamma) * (r - _per_channel(mean)) * _per_channel(invstd) + _per_channel(beta)).reshape(x.shape)
    out = {"mean": mean, "var": var, "invstd": invstd, "z": z, "n": n, "index": None}
    y = z
    if group:
        assert x.ndim == 4 and x.shape[3] == group
        index = np.argmax(z, axis=3)                                # the first maximum; a NaN counts as one
        y = np.take_along_axis(z, index[..., None], 3)[..., 0]
        out["index"] = index
    if relu:
        y = np.where(y <= 0, 0.0, y)                                # (NaN stays NaN)
    out["y"] = y
    out["running_mean"] = out["running_var"] = None
    if running_mean is not None:
        out["running_mean"] = (1 - momentum) * np.asarray(running_mean, f64) + momentum * mean
        out["running_var"] = (1 - momentum) * np.asarray(running_var, f64) + momentum * var * (n / (n - 1.0))
    return out


def backward(x, up, gamma, fwd, relu=True, group=0):
    """``up``: the gradient of forward()'s y -> (dx, dgamma, dbeta) in float64."""
    x = np.asarray(x)
    up = np.asarray(up, dtype=f64)
    g = np.where(fwd["y"] > 0, up, 0.0) if relu else up
    if group:
        full = np.zeros(x.shape, dtype=f64)
        np.put_along_axis(full, fwd["index"][..., None], g[..., None], 3)
        g = full
    r, g = _rows(x), g.reshape(x.shape[0], x.shape[1], -1)
    xhat = (r - _per_channel(fwd["mean"])) * _per_channel(fwd["invstd"])
    dbeta, dgamma = g.sum((0, 2)), (g * xhat).sum((0, 2))
    n = fwd["n"]
    dx = _per_channel(np.asarray(gamma, f64) * fwd["invstd"]) * (g - _per_channel(dbeta / n) - xhat * _per_channel(dgamma / n))
    return dx.reshape(x.shape), dgamma, dbeta


# ---- inputs whose decisions are not marginal -----------------------------------------------------------------------------------
def duplicate_second_half(x):
    """The second half of every group (last axis) repeats the group's element 0: ball-query padding, exact ties."""
    x = np.array(x, copy=True)
    k = x.shape[-1] // 2
    x[..., k:] = x[..., :1]
    return x


def margins(x, gamma, beta, group=0, duplicated=False):
    """-> (the smallest |z|, the smallest gap between the two largest DISTINCT members of a pool group -- inf without pooling).
    ``duplicated``: the group's second half repeats element 0 (checked), so only the first half are distinct members."""
    fwd = forward(x, gamma, beta, relu=False)
    z = fwd["z"]
    zmin = float(np.abs(z).min())
    if not group:
        return zmin, float("inf")
    k = group // 2 if duplicated else group
    if duplicated:
        assert np.array_equal(np.asarray(x)[..., k:], np.broadcast_to(np.asarray(x)[..., :1], np.asarray(x)[..., k:].shape))
        assert np.array_equal(z[..., k:], np.broadcast_to(z[..., :1], z[..., k:].shape))      # same input, same value: an exact tie
    top = np.sort(z[..., :k], axis=-1)
    gap = top[..., -1] - top[..., -2]
    # a whole group of identical inputs (a constant channel) is an exact tie as well
    same = (np.asarray(x)[..., :k] == np.asarray(x)[..., :1]).all(-1)
    gap = np.where(same, np.inf, gap)
    return zmin, float(gap.min())


def check_margins(x, gamma, beta, group=0, duplicated=False):
    zmin, gap = margins(x, gamma, beta, group, duplicated)
    assert zmin >= MARGIN, "a pre-ReLU value within %g of 0: %g" % (MARGIN, zmin)
    assert gap > MARGIN, "two distinct members of a pool group within %g at the top: %g" % (MARGIN, gap)


def enforce_margins(x, gamma, beta, group=0, duplicated=False, rounds=40):
    """Move the few float32 elements of ``x`` that sit within MARGIN of a decision away from it (by 2 MARGIN in z) until
    ``check_margins`` holds; the statistics move with them, hence the rounds.  Channels of identical values are left alone."""
    x = np.array(x, dtype=f32, copy=True)
    gamma64 = np.asarray(gamma, f64)
    assert (np.abs(gamma64) >= 0.25).all()
    for _ in range(rounds):
        fwd = forward(x, gamma, beta, relu=False)
        z = fwd["z"]
        step = (gamma64 * fwd["invstd"]).reshape((1, -1) + (1,) * (x.ndim - 2))          # dz / dx
        dz = np.where(np.abs(z) < 1.5 * MARGIN, np.where(z >= 0, 1.0, -1.0) * (2.5 * MARGIN - np.abs(z)), 0.0)
        if group:
            k = group // 2 if duplicated else group
            order = np.argsort(z[..., :k], axis=-1)
            first, second = order[..., -1:], order[..., -2:-1]
            gap = np.take_along_axis(z, first, -1) - np.take_along_axis(z, second, -1)
            same = (x[..., :k] == x[..., :1]).all(-1, keepdims=True)
            lift = np.where((gap <= 1.5 * MARGIN) & ~same, 2.5 * MARGIN - gap, 0.0)
            cur = np.take_along_axis(dz, first, -1)
            np.put_along_axis(dz, first, np.where(lift > 0, np.maximum(cur, 0.0) + lift, cur), -1)
        if not dz.any():
            break
        x = (x.astype(f64) + dz / step).astype(f32)
        if duplicated:
            x = duplicate_second_half(x)
    check_margins(x, gamma, beta, group, duplicated)
    return x


def affine(C, rng):
    """gamma of both signs with 0.5 <= |gamma| <= 1.5 (the max is taken AFTER the affine), 0.05 <= |beta| <= 0.3 (a constant
    channel's z is beta: off the ReLU threshold), running statistics away from (0, 1)."""
    gamma = (rng.uniform(0.5, 1.5, C) * np.where(rng.random(C) < 0.4, -1.0, 1.0)).astype(f32)
    beta = (rng.uniform(0.05, 0.3, C) * np.where(rng.random(C) < 0.5, -1.0, 1.0)).astype(f32)
    running_mean = rng.standard_normal(C).astype(f32)
    running_var = (rng.random(C) + 0.5).astype(f32)
    return gamma, beta, running_mean, running_var


def upstream(shape, pool, rng):
    """The gradient of y: (B, C, M) with pooling, else x's shape."""
    return rng.standard_normal(shape[:-1] if pool else shape).astype(f32)


def case(shape, pool=0, seed=0):
    """A launch-geometry case: x ~ 0.4 + 1.7 N(0, 1) of ``shape`` ((B, C, L), or (B, C, M, K) with pool = K and the second half
    of every group duplicating element 0) -> dict x, gamma, beta, running_mean, running_var, up; margins enforced."""
    rng = np.random.default_rng(1000 * sum(shape) + pool + seed)
    C = shape[1]
    gamma, beta, rm, rv = affine(C, rng)
    x = (rng.standard_normal(shape) * 1.7 + 0.4).astype(f32)
    if shape[0] * int(np.prod(shape[2:])) == 2:
        # two values per channel: xhat = +-1 nearly whatever they are, z = beta +- gamma -- off the threshold by |gamma| - |beta|
        pair = np.stack([x.reshape(-1)[:C], x.reshape(-1)[:C] + np.where(rng.random(C) < 0.5, -1.0, 1.0)], 1).astype(f32)   # (C, 2)
        x = np.ascontiguousarray(pair.T).reshape(shape) if shape[0] == 2 else pair.reshape(shape)
        check_margins(x, gamma, beta)
    else:
        if pool:
            x = duplicate_second_half(x)
        x = enforce_margins(x, gamma, beta, pool, bool(pool))
    return {"x": x, "gamma": gamma, "beta": beta, "running_mean": rm, "running_var": rv, "up": upstream(shape, pool, rng),
            "pool": pool, "duplicated": bool(pool)}


# (B, C, L) and what it reaches (BN_CHUNK = 8192 elements per apply workgroup, BN_STATS_CHUNK = 32768 per statistics workgroup)
GEOMETRY = [
    (2, 3, 8197),      # L % 4 != 0: the scalar path, 33 elements per thread in the statistics pass, two apply chunks
    (1, 2, 32771),     # scalar path: two statistics chunks, five apply chunks
    (1, 2, 8192),      # vector path, exactly on an apply-chunk edge
    (1, 2, 8196),      # one vector past it
    (2, 2, 32768),     # vector path, exactly on a statistics-chunk edge
    (1, 2, 32772),     # one vector past it
    (3, 129, 40),      # the second finalize block (128 channels each); a ragged last block of bn_partials_reduce_kernel (4 each)
    (2, 3, 1),         # B L = 2, the least torch accepts
    (1, 3, 2),
]
# (B, C, M, K), pool = K
POOLED = [
    (1, 2, 1025, 8),   # group 8, past an apply-chunk edge
    (1, 2, 257, 32),   # group 32, past an apply-chunk edge
    (2, 2, 65, 128),   # group 128, past an apply-chunk edge
    (1, 1, 8193, 4),   # M > 8192: the second block of bn_pool_bwd_reduce_kernel
    (1, 2, 33, 256),   # a last chunk of one group
]
STATS_ONLY = [(2, 3, 8197), (2, 2, 32768)]
NONFINITE = [((2, 4, 300), 0), ((2, 4, 40, 16), 16)]

COND_MEANS = (0.0, 1.0, 10.0, 30.0, 100.0, 300.0, 1000.0, -1000.0)
COND_CONSTANT, COND_ZERO, COND_TINY, COND_WIDE = 8, 9, 10, 11      # channel numbers of the four special channels


def conditioning_case(pool=0, seed=0):
    """(2, 12, 16384), or the same values as (2, 12, 256, 64) with pool = 64: channels 0-7 std 1 at COND_MEANS, then the constant
    100.3, all zeros, std 1e-6 around 0 (variance far below eps) and std 1e4."""
    rng = np.random.default_rng(77 + seed)
    B, C, L = 2, 12, 16384
    gamma, beta, rm, rv = affine(C, rng)
    x = np.empty((B, C, L), dtype=f64)
    for c, m in enumerate(COND_MEANS):
        x[:, c] = m + rng.standard_normal((B, L))
    x[:, COND_CONSTANT] = 100.3
    x[:, COND_ZERO] = 0.0
    x[:, COND_TINY] = 1e-6 * rng.standard_normal((B, L))
    x[:, COND_WIDE] = 1e4 * rng.standard_normal((B, L))
    shape = (B, C, 256, 64) if pool else (B, C, L)
    x = x.astype(f32).reshape(shape)
    x = enforce_margins(x, gamma, beta, pool, False)
    return {"x": x, "gamma": gamma, "beta": beta, "running_mean": rm, "running_var": rv, "up": upstream(shape, pool, rng),
            "pool": pool, "duplicated": False}


def nonfinite_case(shape, pool=0):
    """-> (case, poisoned x): the case's x with one NaN in channel 0 and one +inf in channel 1; channels 2 and 3 untouched."""
    c = case(shape, pool, seed=5)
    bad = np.array(c["x"], copy=True)
    flat = bad.reshape(shape[0], shape[1], -1)          # (a view)
    flat[1, 0, flat.shape[2] // 3] = np.nan
    flat[0, 1, flat.shape[2] - 2] = np.inf
    return c, bad


def conv_stats_inputs(B, Co, Ci, L, ratio, seed=0):
    """x (B, Ci, L), w (Co, Ci) float32 for y = w x whose every output channel has |mean| / std = ``ratio`` (mean +-ratio,
    std 1) up to sampling: x_i = ratio (1 + s e_i) with e ~ N(0, 1), the rows of w = u + sign / Ci with u of unit length and zero
    sum, so that mean_o = sign ratio and std_o = ratio s sqrt(1 + 1 / Ci) = 1."""
    rng = np.random.default_rng(seed + Co + L)
    u = rng.standard_normal((Co, Ci))
    u -= u.mean(1, keepdims=True)
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    sign = np.where(np.arange(Co) % 2 == 0, 1.0, -1.0)[:, None]
    w = (u + sign / Ci).astype(f32)
    s = 1.0 / (ratio * np.sqrt(1.0 + 1.0 / Ci))
    x = (ratio * (1.0 + s * rng.standard_normal((B, Ci, L)))).astype(f32)
    return x, w


def channel_ratio(x, w):
    """|mean| / std of every output channel of y = w x, in float64."""
    y = np.einsum("oi,bil->bol", w.astype(f64), x.astype(f64))
    return np.abs(y.mean((0, 2))) / y.std((0, 2))
