"""Deterministic mode, operator level (torch.use_deterministic_algorithms(True)): every float32 backward equals the
np.add.at restatement (tests/det_reference.py) bit for bit -- small random tables, strided gradients, destinations that
receive nothing, indices out of range, and the real ball-query / 3-NN tables of an 8 x 25 600 training batch (padding
duplicates give one destination hundreds of contributions).  The default atomic kernels add in hardware order, so these
comparisons do not hold without the mode."""
import warnings

import numpy as np
import pytest
import torch

from tests import det_reference as D
from tests.scatter_cases import mixed_grad

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture
def det():
    was, warn = torch.are_deterministic_algorithms_enabled(), torch.is_deterministic_algorithms_warn_only_enabled()
    torch.use_deterministic_algorithms(True)
    try:
        yield
    finally:
        torch.use_deterministic_algorithms(was, warn_only=warn)


_grad = mixed_grad     # values of mixed magnitudes: sums of them depend on the order of the additions


def _bits_equal(a, b):
    a, b = a.detach().cpu().contiguous(), b.detach().cpu().contiguous()
    return a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.mark.parametrize("B,C,N1,N2,K", [(2, 5, 37, 11, 6), (1, 19, 300, 64, 32), (3, 1, 5, 40, 16)])
def test_group_points_backward_small(det, B, C, N1, N2, K):
    from regnet_for_3d_grasping_amd import pn2_ext
    rng = np.random.default_rng(N1)
    idx = torch.from_numpy(rng.integers(-3, N1 + 3, (B, N2, K)))     # out of range on both sides
    idx[:, :, : K // 2] = torch.from_numpy(rng.integers(0, max(N1 // 4, 1), (B, N2, K // 2)))   # crowded destinations
    idx[idx == N1 - 1] = N1 + 1                                      # the last destination receives nothing
    g = _grad(rng, (B, C, N2, K))
    want = D.group_points_backward(g, idx, N1)
    got = pn2_ext.group_points_backward(g.to(DEV), idx.to(DEV), N1)
    assert _bits_equal(got, want)
    assert bool((want[:, :, N1 - 1] == 0).all())   # (written as +0.0)
    # strided grad_output: a (B, C, K, N2) tensor's transposed view
    gt = g.transpose(2, 3).contiguous().to(DEV).transpose(2, 3)
    assert not gt.is_contiguous()
    assert _bits_equal(pn2_ext.group_points_backward(gt, idx.to(DEV), N1), want)


def test_gather_knn_backward_small(det):
    from regnet_for_3d_grasping_amd import dgcnn_ext
    rng = np.random.default_rng(5)
    B, C, N, K = 2, 7, 50, 8
    idx = torch.from_numpy(rng.integers(-1, N + 1, (B, N, K)))
    g = _grad(rng, (B, C, N, K))
    assert _bits_equal(dgcnn_ext.gather_knn_backward(g.to(DEV), idx.to(DEV)), D.gather_knn_backward(g, idx))


@pytest.mark.parametrize("B,C,M,N", [(2, 6, 9, 40), (1, 33, 128, 1000)])
def test_interpolate_backward_small(det, B, C, M, N):
    from regnet_for_3d_grasping_amd import pn2_ext
    rng = np.random.default_rng(M)
    idx = torch.from_numpy(rng.integers(-1, M + 1, (B, N, 3)))
    w = torch.from_numpy(rng.uniform(0, 1, (B, N, 3)).astype(np.float32))
    g = _grad(rng, (B, C, N))
    want = D.interpolate_backward(g, idx, w, M)
    assert _bits_equal(pn2_ext.interpolate_backward(g.to(DEV), idx.to(DEV), w.to(DEV), M), want)
    gt = g.transpose(1, 2).contiguous().to(DEV).transpose(1, 2)
    assert _bits_equal(pn2_ext.interpolate_backward(gt, idx.to(DEV), w.to(DEV), M), want)


def _training_tables():
    """The ball-query tables of levels 1-3 and the 3-NN tables of the three FP blocks of an 8 x 25 600 batch."""
    from regnet_for_3d_grasping_amd import pn2_ext, synthetic
    pc = synthetic.make_batch(8700, 8, 25600).to(DEV)
    xyz = pc[:, :, :3].transpose(1, 2).contiguous()     # (B, N, 6) scenes -> (B, 3, N)
    levels, clouds = [], [xyz]
    for M, r in ((5120, 0.02), (1024, 0.08), (256, 0.32)):
        src = clouds[-1]
        cent = pn2_ext.gather_points(src, pn2_ext.farthest_point_sample(src, M))
        idx, _ = pn2_ext.ball_query(src, cent, r, 64)
        levels.append((idx, src.shape[2]))
        clouds.append(cent.contiguous())
    fps = []
    for dense, sparse in ((clouds[2], clouds[3]), (clouds[1], clouds[2]), (clouds[0], clouds[1])):
        idx, d2 = pn2_ext.point_search(dense, sparse, 3)
        w = 1.0 / (d2 + 1e-8)
        w = (w / w.sum(2, keepdim=True)).contiguous()
        fps.append((idx, w, sparse.shape[2]))
    return levels, fps


def test_training_tables_bit_exact(det):
    from regnet_for_3d_grasping_amd import pn2_ext
    levels, fps = _training_tables()
    rng = np.random.default_rng(11)
    crowded = 0
    for (idx, n1), C in zip(levels, (3, 8, 16)):
        counts = torch.bincount((idx + torch.arange(8, device=DEV).view(8, 1, 1) * n1).view(-1), minlength=8 * n1)
        crowded = max(crowded, int(counts.max()))
        B, N2, K = idx.shape
        g = _grad(rng, (B, C, N2, K))
        got = pn2_ext.group_points_backward(g.to(DEV), idx, n1)
        assert _bits_equal(got, D.group_points_backward(g, idx.cpu(), n1)), (N2, K, n1)
    assert crowded >= 200        # the padding duplicates of sparse balls
    for (idx, w, m), C in zip(fps, (16, 8, 4)):
        B, N, _ = idx.shape
        g = _grad(rng, (B, C, N))
        got = pn2_ext.interpolate_backward(g.to(DEV), idx, w, m)
        assert _bits_equal(got, D.interpolate_backward(g, idx.cpu(), w.cpu(), m)), (N, m)


def test_repeated_calls_give_identical_bytes(det):
    from regnet_for_3d_grasping_amd import pn2_ext
    levels, _ = _training_tables()
    idx, n1 = levels[1]
    g = torch.randn((8, 64) + tuple(idx.shape[1:]), device=DEV)
    a = pn2_ext.group_points_backward(g, idx, n1)
    b = pn2_ext.group_points_backward(g, idx, n1)
    assert _bits_equal(a, b)


def test_one_plan_serves_the_grouping_backward_and_du(det):
    from regnet_for_3d_grasping_amd import pn2_ext
    from regnet_for_3d_grasping_amd.pn2_utils.modules import _GroupMinus
    rng = np.random.default_rng(4)
    B, C, N1, M, K = 2, 12, 200, 50, 16
    idx = torch.from_numpy(rng.integers(0, N1, (B, M, K))).to(DEV)
    g1, g2 = _grad(rng, (B, C, M, K)), _grad(rng, (B, 3, M, K))
    built = pn2_ext.PLANS["built"]
    plan = pn2_ext.scatter_plan(idx, N1)
    a = pn2_ext.group_points_backward(g1.to(DEV), idx, N1, plan)
    b = pn2_ext.group_points_backward(g2.to(DEV), idx, N1, plan)
    assert pn2_ext.PLANS["built"] == built + 1
    assert _bits_equal(a, D.group_points_backward(g1, idx.cpu(), N1))
    assert _bits_equal(b, D.group_points_backward(g2, idx.cpu(), N1))
    with pytest.raises(RuntimeError, match="another table"):
        pn2_ext.group_points_backward(g1.to(DEV), idx.clone(), N1 + 1, plan)
    # the pre-multiplied layer's backward: one plan for dU
    U = torch.randn(B, C, N1, device=DEV, requires_grad=True)
    V = torch.randn(B, C, M, device=DEV, requires_grad=True)
    Y = _GroupMinus.apply(U, V, idx)
    built = pn2_ext.PLANS["built"]
    Y.backward(g1.to(DEV))
    assert pn2_ext.PLANS["built"] == built + 1
    assert _bits_equal(U.grad, D.group_points_backward(g1, idx.cpu(), N1))


def test_scatter_max_grad_bit_exact(det):
    from regnet_for_3d_grasping_amd import region_ops
    rng = np.random.default_rng(9)
    rows, F, R = 300, 24, 1000
    arg = torch.from_numpy(rng.integers(-1, 40, (R, F)))       # 40 of 300 rows take everything; -1: empty group
    dy = _grad(rng, (R, F))
    start = _grad(rng, (rows, F))
    want = D.scatter_max_grad(dy, arg, start.clone())
    got = start.to(DEV)
    region_ops._scatter_max_grad(dy.to(DEV), arg.to(DEV), got, rows, 0, F, 1)
    assert _bits_equal(got, want)
    # channel-first destination (B, F, N): row = b * N + n
    B, N = 3, 100
    got = start.view(B, N, F).transpose(1, 2).contiguous().to(DEV)
    region_ops._scatter_max_grad(dy.to(DEV), arg.to(DEV), got, N, F * N, 1, N)
    assert _bits_equal(got.transpose(1, 2).reshape(rows, F), want)


def test_unsupported_shape_raises_and_warn_only_runs_the_default(det):
    from regnet_for_3d_grasping_amd import determinism, region_ops
    R, F, rows = 8193, 2, 50
    arg = torch.randint(0, rows, (R, F), device=DEV)
    dy = torch.randn(R, F, device=DEV)
    grad = torch.zeros(rows, F, device=DEV)
    with pytest.raises(RuntimeError, match="scatter_max_grad does not have a deterministic implementation"):
        region_ops._scatter_max_grad(dy, arg, grad, rows, 0, F, 1)
    torch.use_deterministic_algorithms(True, warn_only=True)
    determinism._warned.discard("scatter_max_grad")
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        region_ops._scatter_max_grad(dy, arg, grad, rows, 0, F, 1)
        region_ops._scatter_max_grad(dy, arg, grad, rows, 0, F, 1)
    assert len([w for w in seen if "scatter_max_grad" in str(w.message)]) == 1
    want = D.scatter_max_grad(dy.cpu(), arg.cpu(), torch.zeros(rows, F))
    torch.testing.assert_close(grad.cpu(), 2 * want, rtol=1e-5, atol=1e-4)


@pytest.mark.parametrize("pool", [0, 16])
def test_batchnorm_passes_repeat_bitwise(det, pool):
    from regnet_for_3d_grasping_amd import bn_train
    torch.manual_seed(0)
    bn = torch.nn.BatchNorm2d(32).to(DEV).train()
    x = (torch.randn(4, 32, 4096, 16, device=DEV) * 3 + 1).requires_grad_(True)
    runs = []
    for _ in range(2):
        bn.running_mean.zero_(), bn.running_var.fill_(1)
        y = bn_train.bn_relu(bn, x, True, pool)
        g = torch.randn(y.shape, device=DEV, generator=torch.Generator(DEV).manual_seed(1))
        dx, dgamma = torch.autograd.grad(y, (x, bn.weight), g)
        p = bn_train.bn_stats(bn, x.detach())
        runs.append([t.detach().clone() for t in (y, dx, dgamma, bn.running_mean, bn.running_var, p.scale, p.shift)])
    for a, b in zip(*runs):
        assert _bits_equal(a, b)
    # within the default kernels' tolerance of torch's own BatchNorm
    ref = torch.nn.functional.batch_norm(x.detach(), None, None, bn.weight, bn.bias, True, 0.1, bn.eps).clamp_min(0)
    if pool:
        ref = ref.amax(3)
    torch.testing.assert_close(runs[0][0], ref, rtol=1e-4, atol=1e-4)
