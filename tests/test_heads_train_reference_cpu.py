"""tests/heads_train_reference.py, the float64 restatement behind tests/test_gpu_heads_train_edges.py, checked on the CPU: against
torch's own Conv1d -> BatchNorm1d (training) -> ReLU in float64 with autograd, that every input the GPU tests use with ReLU keeps
its decisions away from the margin (check_margins), and the support predicate against the case tables.  The native library is
not loaded here."""
import numpy as np
import pytest
import torch
from torch import nn

from tests import heads_train_reference as H


def _torch64(c, relu, bias=True):
    """torch's modules in float64 on the CPU -> name -> array, the names of H.forward / H.backward."""
    X = torch.from_numpy(c["X"]).double()
    R, K = X.shape
    N = c["W"].shape[0]
    x = X.view(R, K, 1).clone().requires_grad_(True)
    conv = nn.Conv1d(K, N, 1, bias=bias).double()
    bn = nn.BatchNorm1d(N, eps=H.EPS, momentum=H.MOMENTUM).double().train()
    with torch.no_grad():
        conv.weight.copy_(torch.from_numpy(c["W"]).view(N, K, 1))
        if bias:
            conv.bias.copy_(torch.from_numpy(c["bias"]))
        bn.weight.copy_(torch.from_numpy(c["gamma"])), bn.bias.copy_(torch.from_numpy(c["beta"]))
        bn.running_mean.copy_(torch.from_numpy(c["running_mean"])), bn.running_var.copy_(torch.from_numpy(c["running_var"]))
    z = conv(x)
    z.retain_grad()
    y = bn(z)
    if relu:
        y = torch.relu(y)
    y.backward(torch.from_numpy(c["dY"]).double().view(R, N, 1))
    assert int(bn.num_batches_tracked) == 1
    out = {"y": y.view(R, N), "running_mean": bn.running_mean, "running_var": bn.running_var, "dZ": z.grad.view(R, N),
           "dW": conv.weight.grad.view(N, K), "dgamma": bn.weight.grad, "dbeta": bn.bias.grad, "dX": x.grad.view(R, K)}
    if bias:
        out["dbias"] = conv.bias.grad
    return {k: v.detach().numpy() for k, v in out.items()}


def _close(a, b, what, tol=1e-11):
    scale = max(1.0, float(np.abs(b).max()))
    err = float(np.abs(np.asarray(a) - np.asarray(b)).max())
    assert err <= tol * scale, (what, err, scale)


@pytest.mark.parametrize("bias", [True, False])
@pytest.mark.parametrize("relu", [True, False])
@pytest.mark.parametrize("R,K,N", [(2, 64, 5), (3, 64, 1), (37, 128, 17), (129, 64, 40), (300, 256, 33)])
def test_restatement_matches_torch_float64(R, K, N, relu, bias):
    c = H.case(R, K, N, relu)
    b = c["bias"] if bias else None
    fwd = H.forward(c["X"], c["W"], b, c["gamma"], c["beta"], relu, c["running_mean"], c["running_var"], H.MOMENTUM, H.EPS)
    bwd = H.backward(c["X"], c["W"], c["dY"], c["gamma"], fwd, relu)
    want = _torch64(c, relu, bias)
    for name in ("y", "running_mean", "running_var"):
        _close(fwd[name], want[name], name)
    for name in ("dZ", "dW", "dgamma", "dbeta", "dX"):
        _close(bwd[name], want[name], name)
    # the bias in front of a BatchNorm has a zero gradient: rounding noise in both
    scale = max(1.0, float(np.abs(bwd["dZ"]).max()))
    assert float(np.abs(bwd["dbias"]).max()) <= 1e-11 * scale * R
    if bias:
        assert float(np.abs(want["dbias"]).max()) <= 1e-11 * scale * R
        # ... and it enters nothing but the running mean
        none = H.forward(c["X"], c["W"], None, c["gamma"], c["beta"], relu, c["running_mean"], c["running_var"])
        assert np.array_equal(none["y"], fwd["y"]) and np.array_equal(none["running_var"], fwd["running_var"])
        _close(fwd["running_mean"] - none["running_mean"], H.MOMENTUM * c["bias"].astype(np.float64), "bias in running_mean")


def test_two_rows_use_the_unbiased_factor_two():
    c = H.case(2, 64, 3, False)
    fwd = H.forward(c["X"], c["W"], c["bias"], c["gamma"], c["beta"], False, np.zeros(3), np.zeros(3), 1.0, H.EPS)
    _close(fwd["running_var"], 2.0 * fwd["var"], "running_var")
    _close(fwd["running_mean"], fwd["mean"] + c["bias"], "running_mean")


def test_an_explicit_mask_replaces_the_sign_of_y():
    c = H.case(37, 64, 5, True)
    fwd = H.forward(c["X"], c["W"], c["bias"], c["gamma"], c["beta"], True)
    a = H.backward(c["X"], c["W"], c["dY"], c["gamma"], fwd, True)
    b = H.backward(c["X"], c["W"], c["dY"], c["gamma"], fwd, True, mask=fwd["pre"] > 0)
    none = H.backward(c["X"], c["W"], c["dY"], c["gamma"], fwd, True, mask=np.ones(fwd["y"].shape, bool))
    plain = H.backward(c["X"], c["W"], c["dY"], c["gamma"], fwd, False)
    for k in a:
        assert np.array_equal(a[k], b[k]) and np.array_equal(none[k], plain[k]), k
    assert not np.array_equal(a["dZ"], plain["dZ"])


# ---- the GPU test's inputs -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R,K,N", H.geometry_cases() + H.EXTRA_CASES)
def test_geometry_cases_are_not_marginal(R, K, N):
    c = H.case(R, K, N, True)
    assert c["X"].shape == (R, K) and c["W"].shape == (N, K) and c["dY"].shape == (R, N)
    assert all(c[k].dtype == np.float32 for k in ("X", "W", "bias", "gamma", "beta", "running_mean", "running_var", "dY"))
    H.check_margins(c)
    assert float(H.channel_std(c).min()) >= H.MIN_STD, H.channel_std(c).min()
    assert float(np.abs(c["beta"]).max()) < 8.0                      # (the float32 rounding that _GAP allows for)
    fwd = H.forward(c["X"], c["W"], c["bias"], c["gamma"], c["beta"], True)
    if R * N >= 32:
        assert 0.1 < float((fwd["y"] > 0).mean()) < 0.9                  # both branches of the ReLU are taken


@pytest.mark.parametrize("identical", [False, True])
@pytest.mark.parametrize("R", H.CONDITIONING_ROWS)
def test_conditioning_cases_are_what_they_say_and_not_marginal(R, identical):
    c = H.conditioning_case(R, True, identical)
    H.check_margins(c)
    assert bool((c["W"][H.COND_ZERO_ROW] == 0).all())
    std = H.channel_std(c)
    assert std[H.COND_ZERO_ROW] == 0 and (float(std.max()) < 1e-9 if identical else float(np.delete(std, H.COND_ZERO_ROW).min()) >= H.MIN_STD)
    X = c["X"].astype(np.float64)
    if identical:
        assert bool((X == X[:1]).all())
    elif R >= 64:
        for k in range(H.COND_K):
            m = H.COND_MEANS[k % len(H.COND_MEANS)]
            assert abs(X[:, k].mean() - m) < 0.5 and 0.7 < X[:, k].std() < 1.3, k
        ratio = np.delete(H.channel_ratio(c), H.COND_ZERO_ROW)
        assert float(ratio.max()) >= 300.0 and float(np.median(ratio)) >= 30.0, (ratio.max(), np.median(ratio))
    fwd = H.forward(c["X"], c["W"], c["bias"], c["gamma"], c["beta"], True)
    z = H.COND_ZERO_ROW
    assert fwd["var"][z] == 0 and fwd["invstd"][z] == 1.0 / np.sqrt(H.EPS) and bool((fwd["xhat"][:, z] == 0).all())
    assert bool((fwd["pre"][:, z] == np.float64(c["beta"][z])).all())


@pytest.mark.parametrize("relu", [True, False])
def test_low_std_case_is_what_it_says_and_not_marginal(relu):
    c = H.low_std_case(relu)
    assert c["X"].shape == H.LOW_STD_SHAPE[:2] and c["W"].shape == (H.LOW_STD_SHAPE[2], H.LOW_STD_SHAPE[1])
    if relu:
        H.check_margins(c)
    fwd = H.forward(c["X"], c["W"], None, c["gamma"], c["beta"], relu)
    std = np.sqrt(fwd["var"])
    assert 0.9 * H.LOW_STD < std[H.LOW_STD_ROW] < 1.1 * H.LOW_STD and abs(fwd["mean"][H.LOW_STD_ROW] - 1.0) < 0.1
    assert float(np.delete(std, H.LOW_STD_ROW).min()) >= H.MIN_STD


def test_nonfinite_case_poisons_every_channel():
    c, bad = H.nonfinite_case()
    H.check_margins(c)
    assert int(np.isnan(bad).any(1).sum()) == 1 and int(np.isposinf(bad).sum()) == 1
    y = H.forward(bad, c["W"], c["bias"], c["gamma"], c["beta"], True)["y"]
    assert not np.isfinite(y).any()


# ---- regnet_head_layer_train_supported -------------------------------------------------------------------------------------------
def test_supported_covers_the_tables_and_nothing_beyond_the_limits():
    for R in H.ROWS:
        for K, N in H.WIDTHS + [(H.ROWS_K, n) for n in H.ROWS_N]:
            assert H.supported(R, K, N), (R, K, N)
    for R, K, N in H.geometry_cases():
        assert H.supported(R, K, N), (R, K, N)
    for R in (0, 1, 1025):
        assert not H.supported(R, 64, 16), R
    for K in (0, 32, 100):
        assert not H.supported(37, K, 16), K
    assert not H.supported(37, 64, 0)
    assert max(H.ROWS) == H.MAX_ROWS and min(H.ROWS) == 2
    # dynamic LDS of a launch is ceil(R / 16) x 1024 bytes: 928 rows are the last below the launcher's 60000-byte threshold
    lds = lambda R: (R + 15) // 16 * 1024
    assert lds(928) <= 60000 < lds(929) and 928 in H.ROWS and 929 in H.ROWS
    assert lds(1024) + 2368 > 64 * 1024                                    # with the static arrays: beyond 64 KiB
