"""tests/bn_reference.py, the float64 restatement behind tests/test_gpu_bn_train_edges.py, checked on the CPU: against torch's own
BatchNorm1d / BatchNorm2d -> relu -> max in float64 with autograd, its first-maximum rule on duplicated neighbours, and that every
input the GPU tests use keeps its ReLU and arg-max decisions away from the margin (bn_reference.check_margins)."""
import numpy as np
import pytest
import torch
from torch import nn

from tests import bn_reference as R


def _torch64(c, relu, pool):
    """torch's modules in float64 on the CPU -> (y, running_mean, running_var, num_batches_tracked, dx, dgamma, dbeta)."""
    x = torch.from_numpy(c["x"]).double().requires_grad_(True)
    bn = (nn.BatchNorm2d if x.dim() == 4 else nn.BatchNorm1d)(x.shape[1], eps=R.EPS, momentum=R.MOMENTUM).double().train()
    with torch.no_grad():
        bn.weight.copy_(torch.from_numpy(c["gamma"])), bn.bias.copy_(torch.from_numpy(c["beta"]))
        bn.running_mean.copy_(torch.from_numpy(c["running_mean"])), bn.running_var.copy_(torch.from_numpy(c["running_var"]))
    y = bn(x)
    if relu:
        y = torch.relu(y)
    if pool:
        y = torch.max(y, 3)[0]
    y.backward(torch.from_numpy(c["up"]).double())
    return (y.detach().numpy(), bn.running_mean.numpy(), bn.running_var.numpy(), int(bn.num_batches_tracked),
            x.grad.numpy(), bn.weight.grad.numpy(), bn.bias.grad.numpy())


def _mine(c, relu, pool):
    fwd = R.forward(c["x"], c["gamma"], c["beta"], relu, pool, c["running_mean"], c["running_var"])
    return fwd, R.backward(c["x"], c["up"], c["gamma"], fwd, relu, pool)


def _close(a, b, what, tol=1e-12):
    scale = max(1.0, float(np.abs(b).max()))
    err = float(np.abs(np.asarray(a) - np.asarray(b)).max())
    assert err <= tol * scale, (what, err, scale)


@pytest.mark.parametrize("relu", [True, False])
@pytest.mark.parametrize("shape,pool", [((2, 5, 37), 0), ((3, 4, 300), 0), ((2, 3, 1), 0), ((1, 3, 2), 0), ((2, 3, 10, 4), 0),
                                        ((2, 3, 10, 4), 4), ((1, 2, 33, 16), 16)])
def test_restatement_matches_torch_float64(shape, pool, relu):
    rng = np.random.default_rng(sum(shape) + pool)
    gamma, beta, rm, rv = R.affine(shape[1], rng)
    # no duplicated neighbours here: every maximum is unique and torch's choice among ties does not enter
    c = {"x": (rng.standard_normal(shape) * 1.7 + 0.4).astype(np.float32), "gamma": gamma, "beta": beta, "running_mean": rm,
         "running_var": rv, "up": R.upstream(shape, pool, rng)}
    fwd, (dx, dgamma, dbeta) = _mine(c, relu, pool)
    y, run_mean, run_var, nbt, tdx, tdgamma, tdbeta = _torch64(c, relu, pool)
    assert nbt == 1
    _close(fwd["y"], y, "y"), _close(fwd["running_mean"], run_mean, "running_mean"), _close(fwd["running_var"], run_var, "running_var")
    _close(dx, tdx, "dx"), _close(dgamma, tdgamma, "dgamma"), _close(dbeta, tdbeta, "dbeta")


def test_first_maximum_wins_on_duplicated_neighbours():
    c = R.case((2, 3, 9, 8), 8)
    x = c["x"]
    assert np.array_equal(x[..., 4:], np.broadcast_to(x[..., :1], x[..., 4:].shape))
    fwd, (dx, dgamma, dbeta) = _mine(c, True, 8)
    z, index = fwd["z"], fwd["index"]
    top = z.max(-1)
    tied = (z == top[..., None]).sum(-1)
    assert int((tied == 5).sum()) > 0 and int((tied == 1).sum()) > 0      # element 0 wins somewhere: a five-fold tie; and not
    first = np.argmax(z == top[..., None], -1)
    assert np.array_equal(index, first) and bool((index[tied == 5] == 0).all())
    # the whole upstream gradient of a group lands on that one element: take the winner's share out and every element of the
    # group has the same, gradient-free form  -gamma invstd (mean g + xhat mean(g xhat))
    g = np.where(fwd["y"] > 0, c["up"].astype(np.float64), 0.0)
    share = np.zeros_like(z)
    np.put_along_axis(share, index[..., None], g[..., None], 3)
    n = fwd["n"]
    f = (c["gamma"].astype(np.float64) * fwd["invstd"])[None, :, None, None]
    xhat = (x.astype(np.float64) - fwd["mean"][None, :, None, None]) * fwd["invstd"][None, :, None, None]
    rest = -f * (dbeta[None, :, None, None] / n + xhat * dgamma[None, :, None, None] / n)
    _close(dx - f * share, rest, "dx without the winner's share")
    # torch agrees on everything that does not depend on WHICH of the tied elements it picks
    y, _, _, _, tdx, tdgamma, tdbeta = _torch64(c, True, 8)
    _close(fwd["y"], y, "y"), _close(dgamma, tdgamma, "dgamma"), _close(dbeta, tdbeta, "dbeta")
    _close(dx.sum(-1), tdx.sum(-1), "dx summed over a group")


def test_nan_is_a_maximum_and_survives_the_relu():
    x = np.array([[[[1.0, np.nan, 3.0, np.nan], [-1.0, -2.0, -3.0, -4.0]]]], dtype=np.float32)
    z = R.forward(x, [1.0], [0.0], relu=False)["z"]
    assert np.isnan(z).all()                                               # one NaN: the channel's statistics are NaN
    y = np.where(np.array([np.nan, -1.0, 2.0]) <= 0, 0.0, np.array([np.nan, -1.0, 2.0]))
    assert np.isnan(y[0]) and y[1] == 0.0 and y[2] == 2.0
    assert int(np.argmax(np.array([1.0, np.nan, 3.0, np.nan]))) == 1       # the first NaN, like torch.max


@pytest.mark.parametrize("shape", R.GEOMETRY)
def test_geometry_cases_are_not_marginal(shape):
    c = R.case(shape)
    assert c["x"].dtype == np.float32 and c["x"].shape == shape
    R.check_margins(c["x"], c["gamma"], c["beta"])
    assert 0.3 < float(c["x"].mean()) < 0.5 or c["x"].size < 100            # (moving a few elements left the distribution alone)


@pytest.mark.parametrize("shape", R.POOLED)
def test_pooled_cases_are_not_marginal_and_tie_exactly(shape):
    c = R.case(shape, shape[3])
    x = c["x"]
    k = shape[3] // 2
    assert np.array_equal(x[..., k:], np.broadcast_to(x[..., :1], x[..., k:].shape))
    R.check_margins(x, c["gamma"], c["beta"], shape[3], duplicated=True)
    fwd = R.forward(x, c["gamma"], c["beta"], True, shape[3])
    assert int((fwd["index"] == 0).sum()) > 0 and int((fwd["index"] > 0).sum()) > 0   # ties won by element 0, and other winners
    assert int(fwd["index"].max()) < k                                               # never a later duplicate


@pytest.mark.parametrize("pool", [0, 64])
def test_conditioning_case_is_what_it_says_and_not_marginal(pool):
    c = R.conditioning_case(pool)
    x = c["x"].astype(np.float64).reshape(2, 12, -1)
    R.check_margins(c["x"], c["gamma"], c["beta"], pool)
    mean, std = x.mean((0, 2)), x.std((0, 2))
    for ch, m in enumerate(R.COND_MEANS):
        assert abs(mean[ch] - m) < 0.05 and abs(std[ch] - 1.0) < 0.05, (ch, mean[ch], std[ch])
    assert bool((x[:, R.COND_CONSTANT] == np.float32(100.3)).all()) and bool((x[:, R.COND_ZERO] == 0).all())
    assert 0 < std[R.COND_TINY] ** 2 < 1e-3 * R.EPS and abs(mean[R.COND_TINY]) < 1e-5
    assert 0.9e4 < std[R.COND_WIDE] < 1.1e4


@pytest.mark.parametrize("shape,pool", R.NONFINITE)
def test_nonfinite_case_poisons_two_channels_only(shape, pool):
    c, bad = R.nonfinite_case(shape, pool)
    differs = (bad != c["x"]) | np.isnan(bad)
    per_channel = differs.reshape(shape[0], shape[1], -1).sum((0, 2))
    assert per_channel.tolist() == [1, 1, 0, 0]
    assert int(np.isnan(bad).sum()) == 1 and int(np.isposinf(bad).sum()) == 1
    z = R.forward(bad, c["gamma"], c["beta"], True, pool)["y"]
    assert np.isnan(z[:, :2]).all() and np.isfinite(z[:, 2:]).all()


@pytest.mark.parametrize("B,Co,Ci,L", [(3, 160, 64, 4112), (3, 64, 3, 1000)])
@pytest.mark.parametrize("ratio", [10, 30, 100, 1000])
def test_conv_stats_inputs_have_the_ratio_they_claim(B, Co, Ci, L, ratio):
    x, w = R.conv_stats_inputs(B, Co, Ci, L, ratio)
    assert x.dtype == np.float32 and w.dtype == np.float32 and x.shape == (B, Ci, L) and w.shape == (Co, Ci)
    got = R.channel_ratio(x, w)
    assert float(got.min()) > 0.8 * ratio and float(got.max()) < 1.25 * ratio, (float(got.min()), float(got.max()))
