"""fp32-MFMA shared-MLP kernels (csrc/mlp.hip) against a plain PyTorch reference of the same op
(floating-point kernels: tolerance stated per test), plus fused-vs-unfused module equivalence."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _layer(N, K, relu=True, seed=0):
    from regnet_for_3d_grasping_amd import fused
    g = torch.Generator().manual_seed(seed)
    conv = torch.nn.Conv1d(K, N, 1, bias=False)
    bn = torch.nn.BatchNorm1d(N)
    with torch.no_grad():
        conv.weight.copy_(torch.randn(N, K, 1, generator=g) / K ** 0.5)
        bn.weight.copy_(torch.rand(N, generator=g) + 0.5)
        bn.bias.copy_(torch.randn(N, generator=g) * 0.1)
        bn.running_mean.copy_(torch.randn(N, generator=g) * 0.1)
        bn.running_var.copy_(torch.rand(N, generator=g) + 0.5)
    conv, bn = conv.to(DEV), bn.to(DEV).eval()
    return conv, bn, fused._pack(conv, bn, relu)


def _ref(A, conv, bn, relu):
    w = conv.weight.double().squeeze(-1)
    y = A.double() @ w.t()
    y = (y - bn.running_mean.double()) / torch.sqrt(bn.running_var.double() + bn.eps) * bn.weight.double() + bn.bias.double()
    return torch.relu(y) if relu else y


@pytest.mark.parametrize("P,K,N", [(128, 32, 128), (1000, 128, 256), (4096, 260, 128), (777, 516, 384), (64, 1536, 1024)])
def test_mlp_layer_matches_fp64_reference(P, K, N):
    from regnet_for_3d_grasping_amd import fused
    conv, bn, layer = _layer(N, K, seed=P)
    A = torch.randn(P, K, device=DEV)
    got = fused.mlp_layer(A, K, layer, P)
    want = _ref(A, conv, bn, True)
    # fp32 products/accumulation over K<=1536 terms of O(1): 2e-5 absolute is ~10 ulp of the sums
    torch.testing.assert_close(got.double(), want, rtol=1e-5, atol=2e-5)


def test_mlp_layer_asymmetric_identity_and_padding():
    """Transpose-detecting check: A = I (padded), asymmetric W -> C must equal W^T exactly."""
    from regnet_for_3d_grasping_amd import fused
    K, N = 96, 128
    conv = torch.nn.Conv1d(K, N, 1, bias=False).to(DEV)
    with torch.no_grad():
        conv.weight.copy_((torch.arange(N * K, dtype=torch.float32).view(N, K, 1) % 1021) / 7.0)
    layer = fused._pack(conv, None, relu=False)
    A = torch.zeros(200, 100, device=DEV)  # lda 100 > Ka 96
    A[:K, :K] = torch.eye(K, device=DEV)
    A[:, 96:] = 123.0                      # columns >= Ka must be ignored
    got = fused.mlp_layer(A, K, layer, 200)
    assert torch.equal(got[:K], conv.weight.squeeze(-1).t())
    assert float(got[K:].abs().max()) == 0.0


def test_mlp_layer_maxpool_epilogue():
    from regnet_for_3d_grasping_amd import fused
    P, K, N = 64 * 37, 128, 256
    conv, bn, layer = _layer(N, K, seed=3)
    A = torch.randn(P, K, device=DEV)
    got = fused.mlp_layer(A, K, layer, P, pool_group=64)
    want = _ref(A, conv, bn, True).view(37, 64, N).max(dim=1)[0]
    torch.testing.assert_close(got.double(), want, rtol=1e-5, atol=2e-5)


@pytest.mark.parametrize("Cf", [3, 256, 0])
def test_sa_layer1_gather_matches_grouping_reference(Cf):
    from regnet_for_3d_grasping_amd import fused
    B, N, M, G, C1 = 2, 900, 50, 64, 128
    rng = np.random.default_rng(Cf)
    pc = torch.from_numpy(rng.normal(size=(B, N, 3 + max(Cf, 1))).astype(np.float32)).to(DEV)
    xyz = pc[:, :, :3].permute(0, 2, 1)                                  # strided (B,3,N) view
    feat = pc[:, :, 3:3 + Cf].permute(0, 2, 1) if Cf else None           # strided (B,Cf,N) view
    nbr = torch.from_numpy(rng.integers(0, N, (B, M, G))).to(DEV)
    ctr = torch.from_numpy(rng.integers(0, N, (B, M))).to(DEV)
    conv, bn, _ = _layer(C1, 3 + Cf, seed=7)
    order = torch.cat([torch.arange(3, 3 + Cf), torch.arange(3)]).to(DEV)
    layer = fused._pack(conv, bn, True, order)
    got = fused.sa_layer1(feat, xyz, nbr, ctr, layer, B, M, G)
    # reference: the module-level grouping (modules.py:39-56) in torch
    idx = nbr.view(B, 1, M * G)
    gx = torch.gather(xyz, 2, idx.expand(B, 3, -1)).view(B, 3, M, G)
    gx = gx - torch.gather(xyz, 2, ctr[:, None, :].expand(B, 3, M)).unsqueeze(-1)
    parts = [gx]
    if Cf:
        parts.append(torch.gather(feat, 2, idx.expand(B, Cf, -1)).view(B, Cf, M, G))
    grouped = torch.cat(parts, 1).permute(0, 2, 3, 1).reshape(B * M * G, 3 + Cf)
    want = _ref(grouped, conv, bn, True)
    torch.testing.assert_close(got.double(), want, rtol=1e-5, atol=2e-5)


def test_interp_concat_and_score_head():
    from regnet_for_3d_grasping_amd import fused
    from regnet_for_3d_grasping_amd.pointnet2 import PointNet2Seg
    B, Ns, Nd, Cs, Cd = 2, 100, 333, 64, 3
    rng = np.random.default_rng(2)
    sparse = torch.from_numpy(rng.normal(size=(B, Ns, Cs)).astype(np.float32)).to(DEV)
    dense = torch.from_numpy(rng.normal(size=(B, Nd, 6)).astype(np.float32)).to(DEV)[:, :, 3:].permute(0, 2, 1)
    idx = torch.from_numpy(rng.integers(0, Ns, (B, Nd, 3))).to(DEV)
    d2 = torch.from_numpy(rng.uniform(0, 1e-3, (B, Nd, 3)).astype(np.float32)).to(DEV)
    d2[0, 0, 0] = 0.0  # exercises the eps clamp
    out, width = fused.interp_concat(sparse, idx, d2, 1e-10, dense, B, Nd)
    assert width == 68 and tuple(out.shape) == (B * Nd, 68)
    inv = 1.0 / torch.clamp(d2, min=1e-10)
    w = inv / inv.sum(2, keepdim=True)
    g = torch.gather(sparse.unsqueeze(1).expand(B, Nd, Ns, Cs), 2, idx.unsqueeze(-1).expand(B, Nd, 3, Cs))
    want = torch.cat([(g * w.unsqueeze(-1)).sum(2), dense.permute(0, 2, 1), torch.zeros(B, Nd, 1, device=DEV)], 2)
    torch.testing.assert_close(out.view(B, Nd, 68), want, rtol=1e-5, atol=1e-5)

    seg = PointNet2Seg(input_chann=6).to(DEV).eval()
    with torch.no_grad():
        seg.bn_score.running_mean.fill_(0.3)
        seg.bn_score.running_var.fill_(0.7)
        seg.bn_score.weight.fill_(1.7)
    x = torch.randn(500, 128, device=DEV)
    got = fused.score_head(x, seg, 500)
    with torch.no_grad():
        want = torch.sigmoid(seg.bn_score(seg.conv_score(x.t().unsqueeze(0)))).view(-1)
    torch.testing.assert_close(got, want, rtol=1e-5, atol=1e-6)


def test_fused_modules_equal_unfused_modules(monkeypatch):
    """PointNetSAModule / PointnetFPModule: fused MI355X forward == operator-granular forward."""
    import regnet_for_3d_grasping_amd.fused as fused
    from regnet_for_3d_grasping_amd import synthetic
    from regnet_for_3d_grasping_amd.pn2_utils.modules import PointNetSAModule, PointnetFPModule
    torch.manual_seed(0)
    pc = synthetic.make_batch(1005, 2, 4096, device=DEV)
    xyz, rgb = pc.permute(0, 2, 1)[:, :3, :], pc.permute(0, 2, 1)[:, 3:6, :]
    sa = PointNetSAModule(3, (64, 64, 128), 512, 0.05, 64, True).to(DEV).eval()
    fp = PointnetFPModule(128 + 3, (128, 128), 3).to(DEV).eval()
    for m in list(sa.modules()) + list(fp.modules()):
        if isinstance(m, (torch.nn.BatchNorm1d, torch.nn.BatchNorm2d)):
            with torch.no_grad():
                m.running_mean.normal_(0, 0.1)
                m.running_var.uniform_(0.5, 1.5)
                m.weight.uniform_(0.8, 1.2)
                m.bias.normal_(0, 0.1)
    with torch.no_grad():
        monkeypatch.setattr(fused, "ENABLED", True)
        nx1, nf1 = sa(xyz, rgb)
        up1 = fp(xyz, nx1, rgb, nf1)
        monkeypatch.setattr(fused, "ENABLED", False)
        nx0, nf0 = sa(xyz, rgb)
        up0 = fp(xyz, nx0, rgb, nf0)
    assert torch.equal(nx0, nx1)
    assert tuple(nf1.shape) == tuple(nf0.shape) and tuple(up1.shape) == tuple(up0.shape)
    torch.testing.assert_close(nf1, nf0, rtol=1e-4, atol=1e-4)
    torch.testing.assert_close(up1, up0, rtol=1e-4, atol=1e-4)


@pytest.mark.parametrize("pool", [0, 64])
def test_sa_layer12_fused_first_two_layers(pool):
    """Gather + layer 1 (VALU, in the operand load) + layer 2 (MFMA) == the two layers applied in turn."""
    from regnet_for_3d_grasping_amd import fused
    B, N, M, G, C1, C2 = 2, 700, 37, 64, 128, 256
    rng = np.random.default_rng(11)
    pc = torch.from_numpy(rng.normal(size=(B, N, 6)).astype(np.float32)).to(DEV)
    xyz, rgb = pc[:, :, :3].permute(0, 2, 1), pc[:, :, 3:6].permute(0, 2, 1)
    nbr = torch.from_numpy(rng.integers(0, N, (B, M, G))).to(DEV)
    ctr = torch.from_numpy(rng.integers(0, N, (B, M))).to(DEV)
    conv1, bn1, _ = _layer(C1, 6, seed=21)
    conv2, bn2, layer2 = _layer(C2, C1, seed=22)
    order = torch.cat([torch.arange(3, 6), torch.arange(3)]).to(DEV)
    first = fused._pack(conv1, bn1, True, order)
    assert first.W8 is not None and tuple(first.W8.shape) == (C1, 8)
    got = fused.sa_layer12(rgb, xyz, nbr, ctr, first, layer2, B, M, G, pool_group=pool)
    idx = nbr.view(B, 1, M * G)
    gx = torch.gather(xyz, 2, idx.expand(B, 3, -1)).view(B, 3, M, G)
    gx = gx - torch.gather(xyz, 2, ctr[:, None, :].expand(B, 3, M)).unsqueeze(-1)
    gf = torch.gather(rgb, 2, idx.expand(B, 3, -1)).view(B, 3, M, G)
    grouped = torch.cat([gx, gf], 1).permute(0, 2, 3, 1).reshape(B * M * G, 6)
    want = _ref(_ref(grouped, conv1, bn1, True).float(), conv2, bn2, True)
    if pool:
        want = want.view(B * M, G, C2).max(dim=1)[0]
    torch.testing.assert_close(got.double(), want, rtol=1e-5, atol=3e-5)


def test_region_and_refine_heads_fused_equal_torch(monkeypatch):
    import regnet_for_3d_grasping_amd.fused as fused
    from regnet_for_3d_grasping_amd import synthetic
    from regnet_for_3d_grasping_amd.pointnet2 import PointNet2Refine, PointNet2TwoStage
    two = PointNet2TwoStage(256, 6, 4, 40, 4).to(DEV).eval()
    ref = PointNet2Refine(64, 6, 2, 10).to(DEV).eval()
    two.load_state_dict({k: v.to(DEV) for k, v in synthetic.seeded_state_dict(two, 5).items()})
    ref.load_state_dict({k: v.to(DEV) for k, v in synthetic.seeded_state_dict(ref, 6).items()})
    pooled = torch.randn(130, 256, 1, device=DEV)
    grip, region = torch.randn(37, 256, 1, device=DEV), torch.randn(37, 128, device=DEV)
    with torch.no_grad():
        monkeypatch.setattr(fused, "ENABLED", True)
        c1, r1, _ = two(pooled, None, pooled=True)
        a1, b1 = ref(grip, region, pooled=True)
        monkeypatch.setattr(fused, "ENABLED", False)
        c0, r0, _ = two(pooled, None, pooled=True)
        a0, b0 = ref(grip, region, pooled=True)
    for got, want in ((c1, c0), (r1, r0), (a1, a0), (b1, b0)):
        assert got.shape == want.shape
        torch.testing.assert_close(got, want, rtol=1e-4, atol=1e-4)


@pytest.mark.parametrize("n_layers", [2, 3])
def test_sa_premultiplied_first_layer_equals_gathered_form(n_layers, monkeypatch):
    """Wide set-abstraction block: layer 1 evaluated per source point (U[nbr] - V[centre]) == layer 1 over the
    gathered [xyz_j - xyz_c | feature_j] rows (modules.py:44-55), for 2- and 3-layer stacks."""
    import regnet_for_3d_grasping_amd.fused as fused
    from regnet_for_3d_grasping_amd import synthetic
    from regnet_for_3d_grasping_amd.pn2_utils.modules import PointNetSAModule
    torch.manual_seed(3)
    pc = synthetic.make_batch(1010, 2, 3000, device=DEV)
    xyz = pc.permute(0, 2, 1)[:, :3, :]
    feat = torch.randn(2, 128, 3000, device=DEV)
    channels = (128, 256) if n_layers == 2 else (128, 128, 256)
    sa = PointNetSAModule(128, channels, 300, 0.08, 64, True).to(DEV).eval()
    for m in sa.modules():
        if isinstance(m, (torch.nn.BatchNorm1d, torch.nn.BatchNorm2d)):
            with torch.no_grad():
                m.running_mean.normal_(0, 0.1)
                m.running_var.uniform_(0.5, 1.5)
                m.weight.uniform_(0.8, 1.2)
                m.bias.normal_(0, 0.1)
    with torch.no_grad():
        monkeypatch.setattr(fused, "ENABLED", True)
        monkeypatch.setattr(fused, "PREMUL", True)
        nx2, nf2 = sa(xyz, feat)
        monkeypatch.setattr(fused, "PREMUL", False)
        nx1, nf1 = sa(xyz, feat)
        monkeypatch.setattr(fused, "ENABLED", False)
        nx0, nf0 = sa(xyz, feat)
    assert torch.equal(nx0, nx2) and torch.equal(nx1, nx2)
    torch.testing.assert_close(nf2, nf1, rtol=1e-5, atol=2e-5)
    torch.testing.assert_close(nf2, nf0, rtol=1e-4, atol=1e-4)


@pytest.mark.parametrize("Cd", [0, 3, 64])
def test_fp_premultiplied_first_layer_equals_interpolate_then_multiply(Cd, monkeypatch):
    """Feature propagation: W . [interp(sparse) | skip] == interp(Ws . sparse) + Wd . skip (modules.py:117-131)."""
    import regnet_for_3d_grasping_amd.fused as fused
    from regnet_for_3d_grasping_amd import synthetic
    from regnet_for_3d_grasping_amd.pn2_utils.modules import PointnetFPModule
    torch.manual_seed(5)
    pc = synthetic.make_batch(1020, 2, 3000, device=DEV)
    dense_xyz = pc.permute(0, 2, 1)[:, :3, :]
    sparse_xyz = dense_xyz[:, :, ::6].contiguous()
    sparse_feat = torch.randn(2, 256, sparse_xyz.size(2), device=DEV)
    dense_feat = torch.randn(2, Cd, 3000, device=DEV) if Cd else None
    fp = PointnetFPModule(256 + Cd, (256, 128), 3).to(DEV).eval()
    for m in fp.modules():
        if isinstance(m, (torch.nn.BatchNorm1d, torch.nn.BatchNorm2d)):
            with torch.no_grad():
                m.running_mean.normal_(0, 0.1)
                m.running_var.uniform_(0.5, 1.5)
                m.weight.uniform_(0.8, 1.2)
                m.bias.normal_(0, 0.1)
    with torch.no_grad():
        monkeypatch.setattr(fused, "ENABLED", True)
        monkeypatch.setattr(fused, "PREMUL", True)
        up2 = fp(dense_xyz, sparse_xyz, dense_feat, sparse_feat)
        monkeypatch.setattr(fused, "PREMUL", False)
        up1 = fp(dense_xyz, sparse_xyz, dense_feat, sparse_feat)
        monkeypatch.setattr(fused, "ENABLED", False)
        up0 = fp(dense_xyz, sparse_xyz, dense_feat, sparse_feat)
    torch.testing.assert_close(up2, up1, rtol=1e-5, atol=2e-5)
    torch.testing.assert_close(up2, up0, rtol=1e-4, atol=1e-4)


@pytest.mark.parametrize("M,C3,Cf", [(37, 256, 3), (8, 64, 0), (3, 160, 5), (100, 256, 3)])
def test_sa_chain3_whole_block_in_registers(M, C3, Cf):
    """Register-chained level-1 SA block == gather + three (conv, BN, ReLU) layers + max over the 64 neighbours."""
    from regnet_for_3d_grasping_amd import fused
    B, N, G = 2, 900, 64
    rng = np.random.default_rng(31)
    pc = torch.from_numpy(rng.normal(size=(B, N, 3 + max(Cf, 1))).astype(np.float32)).to(DEV)
    xyz = pc[:, :, :3].permute(0, 2, 1)
    feat = pc[:, :, 3:3 + Cf].permute(0, 2, 1) if Cf else None
    nbr = torch.from_numpy(rng.integers(0, N, (B, M, G))).to(DEV)
    ctr = torch.from_numpy(rng.integers(0, N, (B, M))).to(DEV)
    conv1, bn1, _ = _layer(128, Cf + 3, seed=41)
    conv2, bn2, layer2 = _layer(128, 128, seed=42)
    conv3, bn3, layer3 = _layer(C3, 128, seed=43)
    order = torch.cat([torch.arange(3, 3 + Cf), torch.arange(3)]).to(DEV)
    first = fused._pack(conv1, bn1, True, order)
    # ball-query style padding: a neighbourhood with `count` members repeats slot 0 behind them
    count = torch.from_numpy(rng.integers(1, G + 1, (B, M))).to(DEV)
    if M == 100:   # mostly 33..48 members: whole workgroups of paired neighbourhoods (three point tiles per pair), across scenes
        count = torch.from_numpy(rng.choice([33, 40, 47, 48, 48, 41, 36, 20, 49, 64], (B, M))).to(DEV)
    count[0, 0], count[-1, -1] = 32, 33
    slot = torch.arange(G, device=DEV).view(1, 1, G)
    nbr = torch.where(slot < count.unsqueeze(-1), nbr, nbr[:, :, :1].expand(B, M, G)).contiguous()
    order = fused.chain3_order(count)
    got = fused.sa_chain3(feat, xyz, nbr, ctr, first, layer2, layer3, B, M, G, count, order)
    plain = fused.sa_chain3(feat, xyz, nbr, ctr, first, layer2, layer3, B, M, G)
    assert torch.equal(got, plain)     # skipping all-padding point tiles, sharing a tile between two neighbourhoods and reordering change nothing
    # pairs also form without an order (slots w and w + 4 of a workgroup as they come) and under the two-class order
    assert torch.equal(fused.sa_chain3(feat, xyz, nbr, ctr, first, layer2, layer3, B, M, G, count), plain)
    two_class = torch.argsort((count.view(-1) > 32).to(torch.uint8), stable=True)
    assert torch.equal(fused.sa_chain3(feat, xyz, nbr, ctr, first, layer2, layer3, B, M, G, count, two_class), plain)
    idx = nbr.view(B, 1, M * G)
    gx = torch.gather(xyz, 2, idx.expand(B, 3, -1)).view(B, 3, M, G)
    gx = gx - torch.gather(xyz, 2, ctr[:, None, :].expand(B, 3, M)).unsqueeze(-1)
    parts = [gx]
    if Cf:
        parts.append(torch.gather(feat, 2, idx.expand(B, Cf, -1)).view(B, Cf, M, G))
    grouped = torch.cat(parts, 1).permute(0, 2, 3, 1).reshape(B * M * G, Cf + 3)
    h = _ref(_ref(grouped, conv1, bn1, True).float(), conv2, bn2, True).float()
    want = _ref(h, conv3, bn3, True).view(B * M, G, C3).max(dim=1)[0]
    assert tuple(got.shape) == (B * M, C3)
    torch.testing.assert_close(got.double(), want, rtol=1e-5, atol=5e-5)
    # and against the layer-wise kernels
    h2 = fused.sa_layer12(feat, xyz, nbr, ctr, first, layer2, B, M, G)
    want2 = fused.mlp_layer(h2, layer3.K, layer3, B * M * G, pool_group=G)
    torch.testing.assert_close(got, want2, rtol=1e-5, atol=3e-5)


@pytest.mark.parametrize("P,K,N", [(512, 1024, 256), (512, 256, 1024), (300, 128, 40), (64, 1536, 4), (1000, 516, 130)])
def test_mlp_layer_split_k_is_exact_and_deterministic(P, K, N, monkeypatch):
    """Skinny GEMMs take the split-K path: same values as the fp64 reference, bit-identical from run to run, and
    within fp32 round-off of the un-split kernel."""
    from regnet_for_3d_grasping_amd import fused
    conv, bn, layer = _layer(N, K, seed=P + N)
    A = torch.randn(P, (K + 3) // 4 * 4, device=DEV)
    A[:, K:] = 0
    Ka = A.size(1)
    got = fused.mlp_layer(A, Ka, layer, P)
    again = fused.mlp_layer(A, Ka, layer, P)
    assert torch.equal(got, again)
    want = _ref(A[:, :K], conv, bn, True)
    torch.testing.assert_close(got.double(), want, rtol=1e-5, atol=2e-5)
    monkeypatch.setattr(fused, "SPLITK_MAX_ROWS", 0)
    plain = fused.mlp_layer(A, Ka, layer, P)
    torch.testing.assert_close(got, plain, rtol=1e-5, atol=1e-5)


def test_unsupported_configurations_take_the_operator_path(monkeypatch):
    """A set-abstraction block the fused chain does not cover (32 neighbours, one MLP layer) must still run on the GPU
    through the operator-granular kernels -- same result as with the fused path switched off, no exception."""
    import regnet_for_3d_grasping_amd.fused as fused
    from regnet_for_3d_grasping_amd import synthetic
    from regnet_for_3d_grasping_amd.pn2_utils.modules import PointNetSAModule
    torch.manual_seed(2)
    pc = synthetic.make_batch(1030, 2, 2048, device=DEV)
    xyz, rgb = pc.permute(0, 2, 1)[:, :3, :], pc.permute(0, 2, 1)[:, 3:6, :]
    for sa in (PointNetSAModule(3, (32, 64), 128, 0.1, 32, True), PointNetSAModule(3, (48,), 128, 0.1, 64, True)):
        sa = sa.to(DEV).eval()
        assert not fused.supports_sa(sa, rgb)
        with torch.no_grad():
            monkeypatch.setattr(fused, "ENABLED", True)
            nx1, nf1 = sa(xyz, rgb)
            monkeypatch.setattr(fused, "ENABLED", False)
            nx0, nf0 = sa(xyz, rgb)
        assert torch.equal(nx0, nx1) and torch.equal(nf0, nf1)


@pytest.mark.parametrize("P", [128 * 256 + 48, 1000, 16, 7])
def test_fp_head_chain_equals_layerwise_kernels(P):
    """csrc/rowchain.hip (FP3 layers 2-3 + head + score in one kernel) against the same layers run one launch at a
    time, and against an fp64 reference: rows not a multiple of 16 / 128, fewer rows than workgroups, one unit."""
    from regnet_for_3d_grasping_amd import fused, pipeline
    torch.manual_seed(P)
    score_net, _ = pipeline.build_models(DEV)
    seg = score_net.extrat_featurePN2
    seg.bn_score.running_var.fill_(30.0)
    fp = seg.fp_modules[-1]
    assert fused.supports_rowchain(seg, fp)
    fp_layers = fused._packed_stack(fp, fp.mlp)
    h1 = torch.relu(torch.randn(P, 256, device=DEV))
    F, score = fused.fp_head_chain(h1, seg, fp_layers, P)
    # layer-wise
    h = h1
    for layer in fp_layers[1:]:
        h = fused.mlp_layer(h, layer.K, layer, P)
    F_ref = h
    for layer in fused._packed_stack(seg.mlp, seg.mlp):
        h = fused.mlp_layer(h, layer.K, layer, P)
    score_ref = fused.score_head(h, seg, P)
    torch.cuda.synchronize()
    assert torch.isfinite(F).all() and torch.isfinite(score).all()
    torch.testing.assert_close(F, F_ref, rtol=2e-5, atol=2e-5)
    torch.testing.assert_close(score, score_ref, rtol=0, atol=2e-5)
    # fp64 torch reference of the module stack itself (eval mode)
    with torch.no_grad():
        x = h1.double().t()[None]                                       # (1, 256, P)
        mods = [m.double() for m in list(fp.mlp)[1:]]
        for m in mods:
            x = torch.relu(m.bn(m.conv(x)))
        F64 = x[0].t()
        head = [m.double() for m in seg.mlp]
        for m in head:
            x = torch.relu(m.bn(m.conv(x)))
        s64 = torch.sigmoid(seg.bn_score.double()(seg.conv_score.double()(x)))[0, 0]
        score_net.float()
    torch.testing.assert_close(F.double(), F64, rtol=1e-4, atol=1e-4)
    torch.testing.assert_close(score.double(), s64, rtol=0, atol=1e-4)


@pytest.mark.parametrize("B,M", [(2, 64), (1, 33), (3, 1)])
def test_sa_premul_chain_equals_layerwise_kernels(B, M):
    """csrc/rowchain.hip:sa_premul_chain_kernel (level-2 SA block: layers 2 + 3 + pooling in one kernel) against the two
    launches it replaces and an fp64 reference; odd neighbourhood counts (half-filled last block), one neighbourhood."""
    from regnet_for_3d_grasping_amd import fused, pipeline
    torch.manual_seed(10 * B + M)
    score_net, _ = pipeline.build_models(DEV)
    sa = score_net.extrat_featurePN2.sa_modules[1]
    Cf = sa.in_channels
    layers = fused._packed_stack(sa, sa.mlp, lambda: torch.cat([torch.arange(3, 3 + Cf), torch.arange(0, 3)]).to(DEV))
    assert fused.sa_route(sa).features == "premul_chain256"
    Nsrc = 300
    U = torch.randn(B * Nsrc, 256, device=DEV)
    V = torch.randn(B * M, 256, device=DEV) * 0.5
    nbr = torch.randint(0, Nsrc, (B, M, 64), device=DEV)
    got = fused.sa_premul_chain(U, V, nbr, sa, layers, B, Nsrc, M)
    h = fused.sa_premul_layer(U, V, nbr, layers[1], B, Nsrc, M, 64)
    want = fused.mlp_layer(h, layers[2].K, layers[2], B * M * 64, pool_group=64)
    torch.cuda.synchronize()
    assert got.shape == want.shape == (B * M, 512) and torch.isfinite(got).all()
    torch.testing.assert_close(got, want, rtol=2e-5, atol=2e-5)
    with torch.no_grad():
        x0 = torch.relu(U.view(B, Nsrc, 256).double().gather(1, nbr.view(B, M * 64, 1).expand(-1, -1, 256))
                        - V.view(B, M, 1, 256).double().expand(-1, -1, 64, -1).reshape(B, M * 64, 256))
        x = x0.transpose(1, 2).unsqueeze(-1)                       # (B, 256, M*64, 1)
        for blk in list(sa.mlp)[1:]:
            blk = blk.double()
            x = torch.relu(blk.bn(blk.conv(x)))
        ref = x.squeeze(-1).view(B, 512, M, 64).amax(-1).permute(0, 2, 1).reshape(B * M, 512)
        score_net.float()
    torch.testing.assert_close(got.double(), ref, rtol=1e-4, atol=1e-4)


@pytest.mark.parametrize("B,M", [(2, 64), (1, 33), (3, 1), (8, 256)])
def test_sa3_premul_chain_equals_layerwise_kernels(B, M):
    """csrc/rowchain.hip:sa3_premul_chain_kernel (level-3 SA block: 512-wide layers 2 + 3 + pooling in one kernel, layer 2
    as two K-halves) against the two launches it replaces and an fp64 reference; odd neighbourhood counts, one
    neighbourhood, and the bench shape (8 x 256 neighbourhoods = 4 rounds of 256 workgroups)."""
    from regnet_for_3d_grasping_amd import fused, pipeline
    torch.manual_seed(10 * B + M)
    score_net, _ = pipeline.build_models(DEV)
    sa = score_net.extrat_featurePN2.sa_modules[2]
    Cf = sa.in_channels
    layers = fused._packed_stack(sa, sa.mlp, lambda: torch.cat([torch.arange(3, 3 + Cf), torch.arange(0, 3)]).to(DEV))
    assert fused.sa_route(sa).features == "premul_chain512"
    Nsrc = 300
    U = torch.randn(B * Nsrc, 512, device=DEV)
    V = torch.randn(B * M, 512, device=DEV) * 0.5
    nbr = torch.randint(0, Nsrc, (B, M, 64), device=DEV)
    got = fused.sa3_premul_chain(U, V, nbr, sa, layers, B, Nsrc, M)
    h = fused.sa_premul_layer(U, V, nbr, layers[1], B, Nsrc, M, 64)
    want = fused.mlp_layer(h, layers[2].K, layers[2], B * M * 64, pool_group=64)
    torch.cuda.synchronize()
    assert got.shape == want.shape == (B * M, 1024) and torch.isfinite(got).all()
    torch.testing.assert_close(got, want, rtol=2e-5, atol=2e-5)
    if B * M <= 128:
        with torch.no_grad():
            x0 = torch.relu(U.view(B, Nsrc, 512).double().gather(1, nbr.view(B, M * 64, 1).expand(-1, -1, 512))
                            - V.view(B, M, 1, 512).double().expand(-1, -1, 64, -1).reshape(B, M * 64, 512))
            x = x0.transpose(1, 2).unsqueeze(-1)                       # (B, 512, M*64, 1)
            for blk in list(sa.mlp)[1:]:
                blk = blk.double()
                x = torch.relu(blk.bn(blk.conv(x)))
            ref = x.squeeze(-1).view(B, 1024, M, 64).amax(-1).permute(0, 2, 1).reshape(B * M, 1024)
            score_net.float()
        torch.testing.assert_close(got.double(), ref, rtol=1e-4, atol=1e-4)


@pytest.mark.parametrize("B,Nd,Ns", [(2, 1000, 200), (1, 129, 16), (8, 25600, 5120)])
def test_fp_head_chain_interp_equals_interp_affine_then_chain(B, Nd, Ns):
    """fp_head_chain_kernel<true> (first FP layer -- 3-NN interpolation of the pre-multiplied sparse rows + rgb skip + BN +
    ReLU -- in the chain's prologue) against interp_affine_kernel followed by the plain chain: same F and scores up to
    fp32 contraction order; ragged row counts and the bench shape."""
    from regnet_for_3d_grasping_amd import fused, pipeline
    torch.manual_seed(B * 1000 + Nd)
    score_net, _ = pipeline.build_models(DEV)
    seg = score_net.extrat_featurePN2
    fp = seg.fp_modules[-1]
    layers = fused._packed_stack(fp, fp.mlp)
    Cs = layers[0].K - 3
    lay_s, lay_d, wd4 = fused._fp_split_layers(layers[0], Cs)
    assert lay_d is None and wd4 is not None
    Ys = torch.randn(B * Ns, 256, device=DEV)
    idx = torch.randint(0, Ns, (B, Nd, 3), device=DEV)
    dist2 = torch.rand(B, Nd, 3, device=DEV) * 1e-3
    dist2[0, 0, 0] = 0.0                                  # coincident point: the eps clamp
    rgb = torch.rand(B, Nd, 6, device=DEV).permute(0, 2, 1)[:, 3:6, :]   # strided view like the network's
    eps = fp.interpolator._eps
    h1 = fused.interp_affine(Ys, idx, dist2, eps, None, rgb, wd4, layers[0], B, Ns, Nd)
    F_ref, s_ref = fused.fp_head_chain(h1, seg, layers, B * Nd)
    F, s = fused.fp_head_chain_interp(Ys, idx, dist2, eps, rgb, wd4, layers[0], seg, layers, B, Ns, Nd)
    torch.cuda.synchronize()
    assert torch.isfinite(F).all() and torch.isfinite(s).all()
    torch.testing.assert_close(F, F_ref, rtol=2e-5, atol=2e-5)
    torch.testing.assert_close(s, s_ref, rtol=0, atol=2e-5)
    # the partial last round of blocks on a side stream (what ForwardPipeline does): bit-identical rows
    fused.TAIL_SINK = sink = []
    try:
        F2, s2 = fused.fp_head_chain_interp(Ys, idx, dist2, eps, rgb, wd4, layers[0], seg, layers, B, Ns, Nd)
    finally:
        fused.TAIL_SINK = None
    blocks = (B * Nd + 127) // 128
    assert len(sink) == (1 if blocks > 256 and 0 < blocks % 256 <= 128 else 0)
    for ev in sink:
        ev.synchronize()
    torch.cuda.synchronize()
    assert torch.equal(F2, F) and torch.equal(s2, s)


@pytest.mark.parametrize("n", [1, 16, 33, 64, 257, 449, 512, 4000])
def test_heads_chain_kernel_matches_the_layerwise_heads(n):
    """The grasp-region head (7 layers) and the refine head (5 layers) as ONE launch each -- fused.HEADS_CHAIN (csrc/heads.hip
    heads_chain_kernel: 16 rows per workgroup through the whole tree, activations in LDS; the product's path up to 256 rows)
    and fused.HEADS_TREE (heads_tree_kernel: 32 rows per workgroup, the trunk activation chunked; beyond 256 rows, up to the
    4000 centres of test.py:68) -- against each other (same operand mapping and K order: the same bits), against the
    layer-by-layer split-K path and against torch's own modules in float64 (pointnet2.py:174-188, :240-253)."""
    from regnet_for_3d_grasping_amd import fused, synthetic
    from regnet_for_3d_grasping_amd.gripper_region_network import GripperRegionNetwork
    net = GripperRegionNetwork(training=True, group_num=256, gripper_num=64, grasp_score_threshold=0.5, radius=0.06,
                               reg_channel=10)
    net.load_state_dict(synthetic.seeded_state_dict(net, 11))
    net = net.to(DEV).eval()
    g = torch.Generator().manual_seed(n)
    x2 = torch.randn(n, 256, 1, generator=g).to(DEV)
    x3 = torch.randn(n, 384, 1, generator=g).to(DEV)
    outs = {}
    for flag, (chain, tree) in (("chain", (True, False)), ("tree", (False, True)), (False, (False, False))):
        old = (fused.HEADS_CHAIN, fused.HEADS_CHAIN_MAX_ROWS, fused.HEADS_TREE)
        fused.HEADS_CHAIN, fused.HEADS_TREE = chain, tree
        fused.HEADS_CHAIN_MAX_ROWS = 1 << 20          # (the product uses heads_chain_kernel up to 256 rows only)
        try:
            with torch.no_grad():
                outs[flag] = fused.twostage_forward(net.extrat_feature_region, x2) + fused.refine_forward(net.extrat_feature_refine, x3)
        finally:
            fused.HEADS_CHAIN, fused.HEADS_CHAIN_MAX_ROWS, fused.HEADS_TREE = old
    for a, b in zip(outs["tree"], outs["chain"]):
        assert a.shape == b.shape and torch.equal(a, b)
    outs[True] = outs["tree"]
    for a, b in zip(outs[True], outs[False]):
        assert a.shape == b.shape
        torch.testing.assert_close(a, b, rtol=0, atol=2e-5)
    # float64 evaluation of the modules themselves
    import copy
    ref = copy.deepcopy(net).double()
    old, fused.ENABLED = fused.ENABLED, False
    try:
        with torch.no_grad():
            c64, r64, _ = ref.extrat_feature_region(x2.double(), None, pooled=True)
            fc64, fr64 = ref.extrat_feature_refine(x3[:, :256].double(), x3[:, 256:].double().view(n, 128), pooled=True)
    finally:
        fused.ENABLED = old
    for got, want in zip(outs[True], (c64, r64, fc64, fr64)):
        assert float((got.double() - want).abs().max()) <= 2e-5


def test_heads_tree_follows_in_place_weight_updates(monkeypatch):
    """heads_tree_kernel's joined first layer (cls2 | reg2 rows, formal_cls2 | formal_reg2 rows) is part of the named-heads
    pack: tree (512 rows), in-place update, chain (64 rows), in-place update, tree again -- every result equals a freshly
    built network's with the same state_dict, and the second tree call uses a new joined layer (whatever addresses the
    allocator hands the packs of the generation in between)."""
    from regnet_for_3d_grasping_amd import fused, synthetic
    from regnet_for_3d_grasping_amd.gripper_region_network import GripperRegionNetwork

    def build(state=None):
        net = GripperRegionNetwork(training=True, group_num=256, gripper_num=64, grasp_score_threshold=0.5, radius=0.06,
                                   reg_channel=10)
        net.load_state_dict(synthetic.seeded_state_dict(net, 11) if state is None else state)
        return net.to(DEV).eval()

    def run(model, n):
        g = torch.Generator().manual_seed(n)
        x2 = torch.randn(n, 256, 1, generator=g).to(DEV)
        x3 = torch.randn(n, 384, 1, generator=g).to(DEV)
        with torch.no_grad():
            return fused.twostage_forward(model.extrat_feature_region, x2) + fused.refine_forward(model.extrat_feature_refine, x3)

    joined = []
    heads_tree = fused._heads_tree

    def spy(x, L, tree, *args):
        joined.append(L[tree[1]])
        return heads_tree(x, L, tree, *args)

    monkeypatch.setattr(fused, "_heads_tree", spy)
    net = build()
    g = torch.Generator().manual_seed(5)
    stages = []                                      # (rows, outputs, state_dict copy, joined layers used)
    for n in (512, 64, 512):
        if stages:
            with torch.no_grad():                    # an optimizer step's kind of update: in place, same tensors
                for p in net.parameters():
                    p.add_(torch.randn(p.shape, generator=g).to(DEV) * 0.05)
        before = len(joined)
        outs = run(net, n)
        stages.append((n, outs, {k: v.detach().cpu().clone() for k, v in net.state_dict().items()}, joined[before:]))
    assert [len(s[3]) for s in stages] == [2, 0, 2]  # tree, chain, tree (each: region head + refine head)
    for a, b in zip(stages[0][3], stages[2][3]):
        assert a is not b and a.W is not b.W and a.scale is not b.scale and a.shift is not b.shift
    for n, outs, state, _ in stages:
        want = run(build(state), n)
        for a, b in zip(outs, want):
            assert a.shape == b.shape and torch.equal(a, b)
    assert not torch.equal(stages[0][1][0], stages[2][1][0])
