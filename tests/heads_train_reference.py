"""One layer of the grasp heads in TRAINING mode restated in float64 numpy: what csrc/heads_train.hip computes
(regnet_head_layer_train_fwd_f32 / _bwd_f32 / _supported), from the reference's modules (pointnet2.py:174-188, :240-253:
nn.Conv1d(K, N, 1) with bias -> nn.BatchNorm1d(N) on batch statistics -> [ReLU]) -- no import of the package, no GPU.

  forward   z = X W^T;  mean and BIASED variance of a channel over the R rows (two passes);  invstd = 1 / sqrt(var + eps);
            xhat = (z - mean) invstd;  y = [relu](gamma xhat + beta).  The convolution's bias only moves the batch mean:
            running_mean <- (1 - m) running_mean + m (mean + bias),  running_var <- (1 - m) running_var + m var R / (R - 1)
  backward  g = dY where y > 0 (else 0; all of dY without ReLU);  dbeta = sum g;  dgamma = sum g xhat;
            dZ = gamma invstd (g - dbeta / R - xhat dgamma / R);  dW = dZ^T X;  dbias = sum dZ (zero in exact arithmetic);  dX = dZ W

The second half builds float32 inputs.  For a layer with ReLU every DECISION is non-marginal by construction: beta is moved into
the middle of a gap of the channel's sorted gamma * xhat values that is at least 2 MARGIN wide (``check_margins``: |gamma xhat +
beta| >= MARGIN everywhere in float64), so two correct float32 implementations take the same branch at every element and the
gradients are compared element by element.  This is a condition on the inputs, not a tolerance;
tests/test_heads_train_reference_cpu.py asserts it for every case the GPU tests use.
"""
import numpy as np

from tests import bn_reference

f32, f64 = np.float32, np.float64
EPS, MOMENTUM, MARGIN = bn_reference.EPS, bn_reference.MOMENTUM, bn_reference.MARGIN
MAX_ROWS = 1024          # HT_MAX_ROWS: 16 x 1024 floats of LDS per workgroup
COND_MEANS = bn_reference.COND_MEANS


# ---- the operation -----------------------------------------------------------------------------------------------------------
def supported(R, K, N):
    """regnet_head_layer_train_supported."""
    return bool(2 <= R <= MAX_ROWS and K >= 64 and K % 64 == 0 and N >= 1)


def forward(X, W, bias, gamma, beta, relu, running_mean=None, running_var=None, momentum=MOMENTUM, eps=EPS):
    """X (R, K), W (N, K), bias (N,) or None -> dict: z (R, N), mean, var (biased), invstd (N,), xhat, pre (the pre-ReLU values),
    y (R, N), running_mean, running_var (None without the old ones)."""
    X, W = np.asarray(X, f64), np.asarray(W, f64)
    gamma, beta = np.asarray(gamma, f64), np.asarray(beta, f64)
    R = X.shape[0]
    with np.errstate(invalid="ignore", over="ignore"):                  # (a poisoned channel: NaN is the answer)
        z = X @ W.T
        mean = z.sum(0) / R
        var = ((z - mean) ** 2).sum(0) / R                              # two passes: no cancellation
        invstd = 1.0 / np.sqrt(var + eps)
        xhat = (z - mean) * invstd
        pre = gamma * xhat + beta
        y = np.where(pre <= 0, 0.0, pre) if relu else pre               # (NaN stays NaN)
    out = {"z": z, "mean": mean, "var": var, "invstd": invstd, "xhat": xhat, "pre": pre, "y": y, "R": R,
           "running_mean": None, "running_var": None}
    if running_mean is not None:
        shift = mean if bias is None else mean + np.asarray(bias, f64)
        out["running_mean"] = (1 - momentum) * np.asarray(running_mean, f64) + momentum * shift
        out["running_var"] = (1 - momentum) * np.asarray(running_var, f64) + momentum * var * (R / (R - 1.0))
    return out


def backward(X, W, dY, gamma, fwd, relu, mask=None):
    """``dY``: the gradient of forward()'s y; ``mask`` (R, N) bool: where the ReLU passes it (default fwd["y"] > 0)
    -> dict dZ (R, N), dW (N, K), dbias, dgamma, dbeta (N,), dX (R, K) in float64."""
    X, W, g = np.asarray(X, f64), np.asarray(W, f64), np.asarray(dY, f64)
    if relu:
        g = np.where(fwd["y"] > 0 if mask is None else mask, g, 0.0)
    R, xhat = fwd["R"], fwd["xhat"]
    dbeta, dgamma = g.sum(0), (g * xhat).sum(0)
    dZ = np.asarray(gamma, f64) * fwd["invstd"] * (g - dbeta / R - xhat * (dgamma / R))
    return {"dZ": dZ, "dW": dZ.T @ X, "dbias": dZ.sum(0), "dgamma": dgamma, "dbeta": dbeta, "dX": dZ @ W}


# ---- inputs whose decisions are not marginal -----------------------------------------------------------------------------------
# a gap must hold MARGIN on both sides of its middle AFTER beta is rounded to float32 (|beta| < 8: half an ulp is <= 2^-22)
_GAP = 2 * MARGIN + 2.0 ** -20


def _snap_beta(v, threshold):
    """v: the R values gamma * xhat of one channel (float64), ``threshold`` = minus the drawn beta.  -> beta (float32): minus the
    middle of the gap between neighbouring sorted values, at least _GAP wide, whose middle is nearest to the threshold; the two
    open ends count as gaps, with the threshold itself as their point when it lies at least _GAP / 2 outside."""
    s = np.sort(np.asarray(v, f64))
    width = np.diff(s)
    mid = (0.5 * (s[1:] + s[:-1]))[width >= _GAP]
    cand = np.concatenate([mid, [min(threshold, s[0] - 0.5 * _GAP), max(threshold, s[-1] + 0.5 * _GAP)]])
    return f32(-cand[np.argmin(np.abs(cand - threshold))])


def _set_margins(c):
    """Move every channel's beta (drawn already) into the nearest wide gap; in place."""
    fwd = forward(c["X"], c["W"], c["bias"], c["gamma"], c["beta"], False)
    v = c["gamma"].astype(f64) * fwd["xhat"]
    c["beta"] = np.array([_snap_beta(v[:, n], -float(c["beta"][n])) for n in range(v.shape[1])], dtype=f32)
    return c


def margin(c):
    """The smallest |gamma xhat + beta| of a case in float64."""
    fwd = forward(c["X"], c["W"], c["bias"], c["gamma"], c["beta"], False)
    return float(np.abs(fwd["pre"]).min())


def check_margins(c):
    m = margin(c)
    assert m >= MARGIN, "a pre-ReLU value within %g of 0: %g" % (MARGIN, m)


def _affine(N, rng):
    """gamma of both signs with 0.5 <= |gamma| <= 1.5, the drawn beta ~ 0.3 N(0, 1), running statistics away from (0, 1)."""
    gamma = (rng.uniform(0.5, 1.5, N) * np.where(rng.uniform(size=N) < 0.4, -1.0, 1.0)).astype(f32)
    beta = (0.3 * rng.standard_normal(N)).astype(f32)
    return gamma, beta, rng.standard_normal(N).astype(f32), (rng.uniform(size=N) + 0.5).astype(f32)


MIN_STD = 0.3


def _spread(X, W, rng):
    """Draw again the rows of W (~ N(0, 1 / K)) whose channel of z has a batch standard deviation below MIN_STD (two or three rows
    that happen to lie close together): invstd and xhat amplify the rounding of z by 1 / std, so a comparison of two correct fp32
    products below it is a comparison of their roundings.  Measured on an MI355X without this condition: the case (2, 64, 40) with
    ReLU had a channel of std 0.0076 (invstd 132) and its invstd was 3.2e-3 from float64 where torch's own was 3.9e-4 -- above the
    allowed 3 x 3.9e-4 + 132e-5 with nothing wrong in either product; every other case of the tables passed.  A small variance
    beside a large value is tested on purpose instead: ``low_std_case`` (std 1e-2 at a mean of 1, 37 rows) and the conditioning
    cases.  Constant channels (a zero row of W, identical rows of X) stay."""
    X, W = np.asarray(X, f32).astype(f64), np.array(W, dtype=f64)
    for _ in range(200):
        z = X @ W.T
        std, size = z.std(0), np.maximum(1.0, np.abs(z).max(0))
        low = (std < 1.05 * MIN_STD) & (std > 1e-6 * size)
        if not low.any():
            return W
        W[low] = rng.standard_normal((int(low.sum()), W.shape[1])) / np.sqrt(W.shape[1])
    raise AssertionError("no weights with a batch standard deviation of %g in every channel" % MIN_STD)


def channel_std(c):
    """The batch standard deviation of every channel of z in float64."""
    return np.sqrt(forward(c["X"], c["W"], None, c["gamma"], c["beta"], False)["var"])


def _finish(X, W, N, rng, relu, spread=True):
    R = X.shape[0]
    if spread:
        W = _spread(X, W, rng)
    gamma, beta, rm, rv = _affine(N, rng)
    c = {"X": np.ascontiguousarray(X, dtype=f32), "W": np.ascontiguousarray(W, dtype=f32),
         "bias": (0.2 * rng.standard_normal(N)).astype(f32), "gamma": gamma, "beta": beta, "running_mean": rm, "running_var": rv,
         "dY": rng.standard_normal((R, N)).astype(f32), "relu": bool(relu)}
    return _set_margins(c) if relu else c


def case(R, K, N, relu, seed=0):
    """A launch-geometry case: X (R, K) like the output of a ReLU (max(0.3 + N(0, 1), 0): a mean far from zero), W (N, K) ~
    N(0, 1 / K) -> dict X, W, bias, gamma, beta, running_mean, running_var, dY (float32), relu."""
    rng = np.random.RandomState((1000003 * R + 1009 * K + 17 * N + 2 * seed + int(bool(relu))) % (2 ** 32))
    X = np.maximum(0.3 + rng.standard_normal((R, K)), 0.0)
    W = rng.standard_normal((N, K)) / np.sqrt(K)
    return _finish(X, W, N, rng, relu)


COND_K, COND_N, COND_ZERO_ROW = 64, 40, 21       # channel COND_ZERO_ROW has an all-zero row of W: z == 0, a constant channel


def conditioning_case(R, relu, identical=False, seed=0):
    """(R, 64) x (40, 64): column k of X has standard deviation 1 and mean COND_MEANS[k % 8], so that the channels of z = X W^T
    have |mean| / std of several hundred; row COND_ZERO_ROW of W is zero (var == 0, invstd == 1 / sqrt(eps), xhat == 0,
    y == beta).  ``identical``: all R rows of X are its first row (every channel constant)."""
    rng = np.random.RandomState((7919 * R + 31 * seed + 2 * int(bool(identical)) + int(bool(relu)) + 5) % (2 ** 32))
    means = np.array([COND_MEANS[k % len(COND_MEANS)] for k in range(COND_K)], dtype=f64)
    X = means + rng.standard_normal((R, COND_K))
    if identical:
        X = np.repeat(X[:1], R, 0)
    W = rng.standard_normal((COND_N, COND_K)) / np.sqrt(COND_K)
    W[COND_ZERO_ROW] = 0.0
    return _finish(X, W, COND_N, rng, relu)


LOW_STD_SHAPE, LOW_STD_ROW, LOW_STD = (37, 64, 40), 7, 1e-2


def low_std_case(relu):
    """The geometry case (37, 64, 40) with one channel of a small variance beside a large value: row LOW_STD_ROW of W is its drawn
    row scaled to a batch standard deviation of LOW_STD, plus the vector u with (X - mean X) u = 0 and (mean X) u = 1 (37 rows in
    64 dimensions leave room for it) -- z within 0.1 of 1 with a standard deviation of 0.01 in that channel, invstd = 100."""
    R, K, N = LOW_STD_SHAPE
    rng = np.random.RandomState(4242 + int(bool(relu)))
    X = np.maximum(0.3 + rng.standard_normal((R, K)), 0.0).astype(f32).astype(f64)
    W = _spread(X, rng.standard_normal((N, K)) / np.sqrt(K), rng)
    xbar = X.mean(0)
    Xc = X - xbar
    u = np.linalg.pinv(np.vstack([Xc, xbar])) @ np.concatenate([np.zeros(R), [1.0]])
    W[LOW_STD_ROW] = W[LOW_STD_ROW] * (LOW_STD / (Xc @ W[LOW_STD_ROW]).std()) + u
    return _finish(X, W, N, rng, relu, spread=False)


def channel_ratio(c):
    """|mean| / std of every channel of z in float64 (inf for a constant channel)."""
    fwd = forward(c["X"], c["W"], None, c["gamma"], c["beta"], False)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.abs(fwd["mean"]) / np.sqrt(fwd["var"])


def nonfinite_case(R=37, K=64, N=40):
    """-> (case, poisoned X): the case's X with row 5 all NaN and one +inf in row 11; every channel reads both."""
    c = case(R, K, N, True, seed=3)
    bad = np.array(c["X"], copy=True)
    bad[5] = np.nan
    bad[11, K // 2 + 1] = np.inf
    return c, bad


# ---- case tables, shared by the CPU and the GPU test ---------------------------------------------------------------------------
# row counts: the least, both sides of a 16-row tile, of the forward loop's second tile (128 | 129), of its second pass (256 | 257),
# of the launch with more than 64 KiB of LDS (928 | 929: dynamic LDS is ceil(R / 16) KiB, the attribute call starts above 60000 B;
# 944 | 945 the next tile) and of the largest row count
ROWS = [2, 3, 15, 16, 17, 127, 128, 129, 255, 256, 257, 928, 929, 944, 945, 1023, 1024]
ROWS_K, ROWS_N = 64, (1, 16, 40)
# (K, N) of every layer of the shipped heads -- PointNet2TwoStage(k_cls = 4, k_reg = 40), PointNet2Refine(k_cls = 2, k_reg = 10) --
# then partial channel tiles on both sides of 16
SHIPPED_WIDTHS = [(256, 1024), (1024, 256), (256, 128), (128, 4), (128, 40), (384, 1024), (1024, 128), (128, 2), (128, 10)]
WIDTHS = SHIPPED_WIDTHS + [(128, 15), (128, 17)]
WIDTHS_ROWS = (37, 1024)
CONDITIONING_ROWS = (2, 64, 1024)
# cases beside the tables that the GPU test uses with ReLU (leading dimensions, accumulate_dx, optional pointers)
EXTRA_CASES = [(129, 128, 17), (257, 128, 17), (129, 64, 17)]


def geometry_cases():
    """Every (R, K, N) of the two tables, once."""
    out = [(R, ROWS_K, N) for R in ROWS for N in ROWS_N]
    out += [(R, K, N) for (K, N) in WIDTHS for R in WIDTHS_ROWS]
    return out
