"""float64 operators on the MI355X (csrc/ops_f64.hip, csrc/scatter.hip through pn2_ext / dgcnn_ext) against
tests/f64_reference.py: indices, squared distances, gathers and the deterministic backwards compared bit for bit;
gradcheck of the three differentiable autograd Functions; dtype / device errors; float32 still on the float32 kernels."""
import numpy as np
import pytest
import torch

from oracle import pn2_ext_oracle as O

from . import f64_reference as R

pytestmark = pytest.mark.gpu
DEV = "cuda"


def cloud(seed, B, N, lattice=0):
    """(B, 3, N) float64 on the CPU: uniform in a 0.4 m box, or a coarse lattice (many ties and duplicates)."""
    g = torch.Generator().manual_seed(seed)
    if lattice:
        return torch.randint(0, lattice, (B, 3, N), generator=g).double() * 2.0 ** -5
    return torch.rand((B, 3, N), generator=g, dtype=torch.float64) * 0.4 + 0.5


def gpu(*ts):
    return [t.to(DEV) for t in ts]


FPS_CASES = [(1, 2, 2000, 512, 0), (2, 2, 1000, 400, 6), (3, 1, 10, 7, 2), (4, 2, 4100, 1024, 0),
             (5, 1, 25600, 256, 0), (6, 1, 51200, 128, 0)]


@pytest.mark.parametrize("seed,B,N,M,lat", FPS_CASES)
def test_fps_f64_bit_exact(seed, B, N, M, lat):
    x = cloud(seed, B, N, lat)
    want = R.farthest_point_sample(x, M)
    got = x.to(DEV)
    from regnet_for_3d_grasping_amd import pn2_ext
    idx = pn2_ext.farthest_point_sample(got, M)
    assert idx.dtype == torch.int64 and torch.equal(idx.cpu(), want)
    # transposed view of a (B, N, 3) cloud: the same indices
    rows = x.transpose(1, 2).contiguous().to(DEV)
    assert torch.equal(pn2_ext.farthest_point_sample(rows.transpose(1, 2), M).cpu(), want)


BQ_CASES = [(11, 2, 3000, 600, 0.05, 32, 0), (12, 2, 2000, 500, 0.1, 64, 6), (13, 1, 25600, 1024, 0.02, 64, 0),
            (14, 1, 500, 50, 0.3, 16, 0), (15, 1, 5000, 256, 0.01, 64, 0)]


@pytest.mark.parametrize("seed,B,N,M,radius,K,lat", BQ_CASES)
def test_ball_query_f64_bit_exact(seed, B, N, M, radius, K, lat):
    from regnet_for_3d_grasping_amd import pn2_ext
    x = cloud(seed, B, N, lat)
    c = x[:, :, :M].contiguous() + (0.003 if seed == 15 else 0.0)    # seed 15: centroids off the cloud, empty balls too
    wi, wc = R.ball_query(x, c, radius, K)
    gi, gc = pn2_ext.ball_query(*gpu(x, c), radius, K)
    assert gi.dtype == torch.int64 and gc.dtype == torch.int64
    assert torch.equal(gi.cpu(), wi) and torch.equal(gc.cpu(), wc)
    xt = x.transpose(1, 2).contiguous().to(DEV).transpose(1, 2)
    ct = c.transpose(1, 2).contiguous().to(DEV).transpose(1, 2)
    gi, gc = pn2_ext.ball_query(xt, ct, radius, K)
    assert torch.equal(gi.cpu(), wi) and torch.equal(gc.cpu(), wc)


NN_CASES = [(21, 2, 3000, 700, 0), (22, 2, 1000, 250, 5), (23, 1, 25600, 5120, 0), (24, 1, 7, 3, 0)]


@pytest.mark.parametrize("seed,B,N1,N2,lat", NN_CASES)
def test_three_nn_f64_bit_exact(seed, B, N1, N2, lat):
    from regnet_for_3d_grasping_amd import pn2_ext
    q = cloud(seed, B, N1, lat)
    k = cloud(seed + 100, B, N2, lat)
    wi, wd = R.point_search(q, k, 3)
    gi, gd = pn2_ext.point_search(*gpu(q, k), 3)
    assert gd.dtype == torch.float64
    assert torch.equal(gi.cpu(), wi) and torch.equal(gd.cpu(), wd)
    qt = q.transpose(1, 2).contiguous().to(DEV).transpose(1, 2)
    gi, gd = pn2_ext.point_search(qt, k.to(DEV), 3)
    assert torch.equal(gi.cpu(), wi) and torch.equal(gd.cpu(), wd)


def _indices(kind, B, N1, N2, K, seed):
    g = torch.Generator().manual_seed(seed)
    if kind == "random":
        return torch.randint(0, N1, (B, N2, K), generator=g)
    if kind == "padded":      # ball-query padding: each row repeats its first member after a few hits
        x = cloud(seed, B, N1)
        return R.ball_query(x, x[:, :, :N2].contiguous(), 0.03, K)[0]
    return torch.zeros((B, N2, K), dtype=torch.int64)      # every source on one destination


# backward kernels in double (csrc/scatter.hip): one LDS chunk; several LDS chunks; several LDS chunks, nine channels;
# 20 000 destinations, whose state does not fit in LDS -> the global-memory kernel; one chunk staging 8 channels per
# workgroup (the last block 6)
@pytest.mark.parametrize("kind", ["random", "padded", "collide"])
@pytest.mark.parametrize("B,C,N1,N2,K", [(2, 7, 500, 128, 16), (1, 3, 5000, 1024, 64), (2, 9, 2000, 640, 64),
                                         (1, 5, 20000, 1024, 32), (4, 1030, 500, 128, 16)])
def test_group_points_f64_bit_exact(kind, B, C, N1, N2, K):
    from regnet_for_3d_grasping_amd import dgcnn_ext, pn2_ext
    gen = torch.Generator().manual_seed(N1 + K)
    x = torch.randn((B, C, N1), generator=gen, dtype=torch.float64)
    idx = _indices(kind, B, N1, N2, K, 31)
    g = torch.randn((B, C, N2, K), generator=gen, dtype=torch.float64)
    xd, idxd, gd = gpu(x, idx, g)
    fwd = pn2_ext.group_points_forward(xd, idxd)
    assert fwd.dtype == torch.float64 and torch.equal(fwd.cpu(), R.group_points_forward(x, idx))
    assert torch.equal(pn2_ext.group_points_forward(x.transpose(1, 2).contiguous().to(DEV).transpose(1, 2), idxd).cpu(),
                       fwd.cpu())
    want = R.group_points_backward(g, idx, N1)
    b1 = pn2_ext.group_points_backward(gd, idxd, N1)
    b2 = pn2_ext.group_points_backward(gd, idxd, N1)
    assert torch.equal(b1.cpu(), want) and torch.equal(b1, b2)
    # strided grad_output (a permuted view) and the dgcnn_ext surface
    gt = g.permute(0, 3, 1, 2).contiguous().to(DEV).permute(0, 2, 3, 1)
    assert torch.equal(pn2_ext.group_points_backward(gt, idxd, N1).cpu(), want)
    if N1 == N2:
        assert torch.equal(dgcnn_ext.gather_knn_backward(gd, idxd).cpu(), want)


@pytest.mark.parametrize("kind", ["random", "padded", "collide"])
def test_gather_knn_f64_bit_exact(kind):
    from regnet_for_3d_grasping_amd import dgcnn_ext
    B, C, N, K = 2, 5, 400, 8
    gen = torch.Generator().manual_seed(5)
    x = torch.randn((B, C, N), generator=gen, dtype=torch.float64)
    idx = _indices(kind, B, N, N, K, 41)
    g = torch.randn((B, C, N, K), generator=gen, dtype=torch.float64)
    xd, idxd, gd = gpu(x, idx, g)
    assert torch.equal(dgcnn_ext.gather_knn_forward(xd, idxd).cpu(), R.gather_knn_forward(x, idx))
    b1, b2 = dgcnn_ext.gather_knn_backward(gd, idxd), dgcnn_ext.gather_knn_backward(gd, idxd)
    assert torch.equal(b1.cpu(), R.gather_knn_backward(g, idx)) and torch.equal(b1, b2)


# backward kernels in double: one LDS chunk; several LDS chunks; one chunk; the global-memory kernel (12 000 destinations
# and 20 000 slots); one chunk staging 4 channels per workgroup (the last block 2)
@pytest.mark.parametrize("B,C,M,N,kind", [(2, 9, 300, 1200, "nn"), (1, 4, 5120, 25600, "nn"), (2, 3, 50, 700, "collide"),
                                          (1, 3, 12000, 20000, "random"), (2, 1030, 300, 1200, "nn")])
def test_interpolate_f64_bit_exact(B, C, M, N, kind):
    from regnet_for_3d_grasping_amd import pn2_ext
    gen = torch.Generator().manual_seed(M)
    x = torch.randn((B, C, M), generator=gen, dtype=torch.float64)
    if kind == "nn":
        idx, d2 = R.point_search(cloud(1, B, N), cloud(2, B, M), 3)
        inv = 1.0 / torch.clamp(d2, min=1e-10)
        w = inv / inv.sum(2, keepdim=True)
    else:
        idx = torch.zeros((B, N, 3), dtype=torch.int64)
        if kind == "random":
            idx = torch.randint(0, M, (B, N, 3), generator=gen)
        w = torch.rand((B, N, 3), generator=gen, dtype=torch.float64)
    g = torch.randn((B, C, N), generator=gen, dtype=torch.float64)
    xd, idxd, wd, gd = gpu(x, idx, w, g)
    fwd = pn2_ext.interpolate_forward(xd, idxd, wd)
    assert fwd.dtype == torch.float64 and torch.equal(fwd.cpu(), R.interpolate_forward(x, idx, w))
    want = R.interpolate_backward(g, idx, w, M)
    b1, b2 = pn2_ext.interpolate_backward(gd, idxd, wd, M), pn2_ext.interpolate_backward(gd, idxd, wd, M)
    assert torch.equal(b1.cpu(), want) and torch.equal(b1, b2)
    gt = g.transpose(1, 2).contiguous().to(DEV).transpose(1, 2)
    assert torch.equal(pn2_ext.interpolate_backward(gt, idxd, wd, M).cpu(), want)


def test_gradcheck_autograd_functions():
    from regnet_for_3d_grasping_amd.pn2_utils import function as F
    from regnet_for_3d_grasping_amd.pn2_utils.functions.gather_knn import GatherKNN
    gen = torch.Generator().manual_seed(3)
    x = torch.randn((2, 3, 12), generator=gen, dtype=torch.float64).to(DEV).requires_grad_()
    idx = torch.randint(0, 12, (2, 5, 4), generator=gen)
    idx[0, 0] = 7                                             # collisions in one row
    idx = idx.to(DEV)
    assert torch.autograd.gradcheck(lambda f: F.GroupPoints.apply(f, idx), (x,))
    # gather_knn's backward sizes grad_input by the index rows (gather_knn_kernel.cu:100-153): one row per point
    kidx = torch.randint(0, 12, (2, 12, 4), generator=gen)
    kidx[1, :, 0] = 3
    assert torch.autograd.gradcheck(lambda f: GatherKNN.apply(f, kidx.to(DEV)), (x,))
    nidx = torch.randint(0, 12, (2, 9, 3), generator=gen).to(DEV)
    w = torch.rand((2, 9, 3), generator=gen, dtype=torch.float64).to(DEV)
    assert torch.autograd.gradcheck(lambda f: F.FeatureInterpolate.apply(f, nidx, w), (x,))


def test_dtype_and_device_errors():
    from regnet_for_3d_grasping_amd import dgcnn_ext, pn2_ext
    x64 = torch.rand((1, 3, 40), dtype=torch.float64, device=DEV)
    x32, x16 = x64.float(), x64.half()
    idx = torch.zeros((1, 4, 2), dtype=torch.int64, device=DEV)
    nidx = torch.zeros((1, 40, 3), dtype=torch.int64, device=DEV)
    calls = [lambda: pn2_ext.ball_query(x64, x32, 0.1, 4), lambda: pn2_ext.ball_query(x32, x64, 0.1, 4),
             lambda: pn2_ext.point_search(x64, x32, 3), lambda: pn2_ext.point_search(x32, x64, 3),
             lambda: pn2_ext.interpolate_forward(x64, nidx, nidx.float()),
             lambda: pn2_ext.interpolate_forward(x32, nidx, nidx.double()),
             lambda: pn2_ext.interpolate_backward(x64, nidx, nidx.float(), 40),
             lambda: pn2_ext.farthest_point_sample(x16, 4), lambda: pn2_ext.ball_query(x16, x16, 0.1, 4),
             lambda: pn2_ext.point_search(x16, x16, 3), lambda: pn2_ext.group_points_forward(x16, idx),
             lambda: pn2_ext.group_points_backward(torch.zeros((1, 3, 4, 2), dtype=torch.half, device=DEV), idx, 40),
             lambda: dgcnn_ext.gather_knn_forward(x16, idx),
             lambda: pn2_ext.farthest_point_sample(x64.cpu(), 4), lambda: pn2_ext.group_points_forward(x64.cpu(), idx.cpu()),
             lambda: pn2_ext.farthest_point_sample(x64, 4, pn2_ext.FpsChain())]
    for call in calls:
        with pytest.raises(RuntimeError):
            call()
    with pytest.raises(RuntimeError, match="float32 or float64"):
        pn2_ext.group_points_forward(x16, idx)


def test_float32_stays_on_the_float32_kernels():
    from regnet_for_3d_grasping_amd import dgcnn_ext, pn2_ext
    x = cloud(7, 2, 3000).float()
    c = x[:, :, :500].contiguous()
    xd, cd = gpu(x, c)
    idx = pn2_ext.farthest_point_sample(xd, 300)
    assert torch.equal(idx.cpu(), O.farthest_point_sample(x, 300))
    bi, bc = pn2_ext.ball_query(xd, cd, 0.05, 32)
    wi, wc = O.ball_query(x, c, 0.05, 32)
    assert torch.equal(bi.cpu(), wi) and torch.equal(bc.cpu(), wc)
    ni, nd = pn2_ext.point_search(xd, cd, 3)
    wi, wd = O.point_search(x, c, 3)
    assert nd.dtype == torch.float32 and torch.equal(ni.cpu(), wi) and torch.equal(nd.cpu(), wd)
    f = torch.randn(2, 6, 3000)
    g = pn2_ext.group_points_forward(f.to(DEV), bi)
    assert g.dtype == torch.float32 and torch.equal(g.cpu(), O.group_points_forward(f, bi.cpu()))
    assert torch.equal(dgcnn_ext.gather_knn_forward(f.to(DEV), bi).cpu(), g.cpu())
    w = torch.rand(2, 3000, 3)
    out = pn2_ext.interpolate_forward(f[:, :, :500].contiguous().to(DEV), ni, w.to(DEV))
    assert out.dtype == torch.float32      # (the float32 kernel may contract x*w + acc: equal up to that rounding)
    torch.testing.assert_close(out.cpu(), O.interpolate_forward(f[:, :, :500].contiguous(), ni.cpu(), w), rtol=1e-6, atol=1e-6)
    gb = pn2_ext.group_points_backward(torch.ones(2, 6, 500, 32, device=DEV), bi, 3000)
    assert gb.dtype == torch.float32      # integer-valued sums: exact in any order
    assert torch.equal(gb.cpu(), O.group_points_backward(torch.ones(2, 6, 500, 32), bi.cpu(), 3000))
