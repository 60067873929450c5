"""The float64 restatements of tests/mlp_modes_reference.py against independent restatements (explicit Python loops for the
operands, torch's own gather / Conv1d / BatchNorm1d in float64 for the layers), the exactness of the exact-mode inputs, the
bounds, and the case tables of tests/mlp_modes_cases.py against the edges they are there for and against the tile constants
of csrc/mlp.hip.  No GPU."""
import os
import re

import pytest
import torch

from . import mlp_modes_cases as cases
from . import mlp_modes_reference as ref

CPU = "cpu"
MLP_HIP = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "regnet_for_3d_grasping_amd", "csrc", "mlp.hip")


def test_tile_constants_match_the_kernel_source():
    with open(MLP_HIP) as f:
        text = f.read()

    def define(name):
        found = re.findall(r"^#define[ \t]+%s[ \t]+(\d+)\b" % name, text, flags=re.M)
        assert len(found) == 1, (name, found)
        return int(found[0])
    assert (define("BM"), define("BN"), define("MLP_BK"), define("IC_ROWS")) == (cases.BM, cases.BN, cases.BK, cases.IC_ROWS)
    assert re.search(r"^#define[ \t]+BK[ \t]+MLP_BK\b", text, flags=re.M)
    assert define("MLP_THREADS") == cases.GLUE_THREADS


# ---- the tables ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [1, 2, 3])
def test_sa_table_reaches_every_edge(mode):
    rows = [c for c in cases.SA_CASES if c.mode == mode]
    have = set().union(*(cases.sa_tags(c) for c in rows))
    assert cases.SA_REQUIRED[mode] <= have, sorted(cases.SA_REQUIRED[mode] - have)


def test_sa_table_is_well_formed_and_small():
    assert len({c.id for c in cases.SA_CASES}) == len(cases.SA_CASES)
    for c in cases.SA_CASES:
        assert 1 <= cases.sa_rows(c) <= 2048 and c.ldc_pad in (1, 4) and c.relu in (0, 1) and c.pool in (0, 64), c.id
        assert not c.pool or (c.group == 64 and c.mode != 1), c.id
        assert cases.sa_kpad(c) % cases.BK == 0, c.id
        if c.mode == 1:
            assert (c.feat == "none") == (c.Cf == 0) and c.Cf + 3 <= cases.sa_kpad(c), c.id
        if c.mode == 2:
            assert c.Cf + 3 <= 8 and c.C1 % cases.BK == 0 and c.C1 <= 256 and c.feat == ("cfirst" if c.Cf else "none"), c.id
        if c.mode == 3:
            assert c.C1 % 4 == 0, c.id
        if "extremes" in c.opts:
            assert c.M >= 2, c.id
    # a ragged last k-tile in mode 3, and a pooled last tile of one neighbourhood in both pooled modes
    assert any(c.mode == 3 and c.C1 % cases.BK for c in cases.SA_CASES)


def test_glue_tables_reach_every_edge():
    for table, tags, required in ((cases.IC_CASES, cases.ic_tags, cases.IC_REQUIRED), (cases.IA_CASES, cases.ia_tags, cases.IA_REQUIRED),
                                  (cases.SH_CASES, cases.sh_tags, cases.SH_REQUIRED)):
        have = set().union(*(tags(c) for c in table))
        assert required <= have, sorted(required - have)
        assert len({c.id for c in table}) == len(table)
    for c in cases.IC_CASES:
        assert c.Cout >= c.Cs + c.Cd and c.B * c.Nd <= 2048 and (c.dense == "none") == (c.Cd == 0), c.id
    for c in cases.IA_CASES:
        assert c.C % 4 == 0 and 256 % (c.C // 4) == 0 and c.B * c.Nd <= 2048 and 0 <= c.Cds <= 4, c.id
    assert [C for C, _ in cases.IA_REFUSALS] == [6, 12]


# ---- the reference against independent restatements -----------------------------------------------------------------------
def _tiny_sa(mode, **kw):
    base = dict(id="tiny", mode=mode, B=2, M=3, group=4, Nsrc=5, N=6, Cf=0, C1=0, feat="none", kx=0, pool=0, relu=1, ldc_pad=1,
                opts=frozenset(("extremes",)))
    base.update(kw)
    return cases.Sa(**base)


@pytest.mark.parametrize("layout", ["clast", "cfirst", "offset"])
def test_gather_operand_equals_an_explicit_loop(layout):
    c = _tiny_sa(1, Cf=5, feat=layout)
    d = ref.sa_inputs(c, False, 1, CPU)
    got = ref.gather_operand(d["feat"], d["xyz"], d["nbr"], d["ctr"], c.B, c.M, c.group, c.Cf)
    assert got.dtype == torch.float32 and tuple(got.shape) == (c.B * c.M * c.group, c.Cf + 3)
    for b in range(c.B):
        for m in range(c.M):
            for k in range(c.group):
                j, cj = int(d["nbr"][b, m, k]), int(d["ctr"][b, m])
                row = got[(b * c.M + m) * c.group + k]
                assert torch.equal(row[:c.Cf], d["feat"][b, j])
                for a in range(3):
                    assert float(row[c.Cf + a]) == float(d["xyz"][b, a, j] - d["xyz"][b, a, cj])
    no_feat = ref.gather_operand(None, d["xyz"], d["nbr"], d["ctr"], c.B, c.M, c.group, 0)
    assert torch.equal(no_feat, got[:, c.Cf:])


def test_premul_operand_equals_an_explicit_loop():
    c = _tiny_sa(3, C1=8)
    d = ref.sa_inputs(c, False, 2, CPU)
    assert d["U"].shape[1] == c.C1 + 4 and bool(torch.isnan(d["U"][:, c.C1:]).all()) and bool(torch.isnan(d["V"][:, c.C1:]).all())
    got = ref.premul_operand(d["U"], d["V"], d["nbr"], c.B, c.Nsrc, c.M, c.group, c.C1)
    assert got.dtype == torch.float32 and bool(torch.isfinite(got).all())
    nbr = d["nbr"].reshape(-1)
    for p in range(c.B * c.M * c.group):
        b = p // (c.M * c.group)
        for k in range(c.C1):
            want = max(float(d["U"][b * c.Nsrc + int(nbr[p]), k] - d["V"][p // c.group, k]), 0.0)
            assert float(got[p, k]) == want


def _conv_bn(w, scale, shift):
    """(conv, bn) float64 modules in eval mode computing scale * (w . x) + shift (running_var + eps == 1)."""
    N, K = w.shape
    conv = torch.nn.Conv1d(K, N, 1, bias=False).double()
    bn = torch.nn.BatchNorm1d(N).double().eval()
    with torch.no_grad():
        conv.weight.copy_(w.double().unsqueeze(-1))
        bn.running_mean.zero_()
        bn.running_var.fill_(1.0 - bn.eps)
        bn.weight.copy_(scale.double())
        bn.bias.copy_(shift.double())
    return conv, bn


def _module_layer(rows, w, scale, shift, relu):
    conv, bn = _conv_bn(w, scale, shift)
    with torch.no_grad():
        y = bn(conv(rows.double().t().unsqueeze(0)))[0].t()
    return torch.relu(y) if relu else y


def _grouped(d, c):
    """The module-level grouping of tests/test_gpu_mlp.py: torch.gather on (B, C, N) tensors, [feat | xyz - centre] rows."""
    B, M, G = c.B, c.M, c.group
    idx = d["nbr"].view(B, 1, M * G)
    gx = torch.gather(d["xyz"], 2, idx.expand(B, 3, -1)).view(B, 3, M, G)
    gx = gx - torch.gather(d["xyz"], 2, d["ctr"][:, None, :].expand(B, 3, M)).unsqueeze(-1)
    parts = [gx]
    if c.Cf:
        parts.insert(0, torch.gather(d["feat"].permute(0, 2, 1), 2, idx.expand(B, c.Cf, -1)).view(B, c.Cf, M, G))
    return torch.cat(parts, 1).permute(0, 2, 3, 1).reshape(B * M * G, c.Cf + 3)


@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("Cf", [0, 5])
def test_gather_layer_equals_torch_modules(Cf, relu):
    c = _tiny_sa(1, Cf=Cf, feat="cfirst" if Cf else "none")
    d = ref.sa_inputs(c, False, 3, CPU)
    y, tol, _ = ref.sa_reference(c, d, relu, cases.sa_kpad(c))
    want = _module_layer(_grouped(d, c), d["w"], d["scale"], d["shift"], relu)
    torch.testing.assert_close(y, want, rtol=1e-12, atol=1e-12)
    assert tol.shape == y.shape


@pytest.mark.parametrize("pool", [0, 64])
def test_layer12_equals_two_torch_modules(pool):
    c = _tiny_sa(2, Cf=5, C1=16, feat="cfirst", group=64, pool=pool, M=2)
    d = ref.sa_inputs(c, False, 4, CPU)
    y, tol, _ = ref.sa_reference(c, d, 1, cases.sa_kpad(c))
    h = _module_layer(_grouped(d, c), d["w1"], d["scale1"], d["shift1"], 1)
    want = _module_layer(h, d["w"], d["scale"], d["shift"], 1)
    if pool:
        want = want.view(c.B * c.M, 64, c.N).max(dim=1)[0]
    torch.testing.assert_close(y, want, rtol=1e-12, atol=1e-12)
    assert tol.shape == y.shape
    # the propagated layer-1 error is part of the bound: it exceeds layer 2's own
    x = ref.gather_operand(d["feat"], d["xyz"], d["nbr"], d["ctr"], c.B, c.M, c.group, c.Cf)
    own = ref.layer(torch.relu(h).float(), c.C1, d["w"], d["scale"], d["shift"], 1, pool, cases.sa_kpad(c))[1]
    assert bool((tol > own * 0.999).all()) and x.shape[1] == 8


@pytest.mark.parametrize("pool", [0, 64])
def test_premul_layer_equals_torch_modules(pool):
    c = _tiny_sa(3, C1=8, group=64, M=2, pool=pool)
    d = ref.sa_inputs(c, False, 5, CPU)
    y, _, _ = ref.sa_reference(c, d, 1, cases.sa_kpad(c))
    B, M, G, C1 = c.B, c.M, c.group, c.C1
    x0 = torch.relu((d["U"][:, :C1].view(B, c.Nsrc, C1).gather(1, d["nbr"].view(B, M * G, 1).expand(-1, -1, C1))
                     - d["V"][:, :C1].view(B, M, 1, C1).expand(-1, -1, G, -1).reshape(B, M * G, C1))).reshape(B * M * G, C1)
    want = _module_layer(x0, d["w"], d["scale"], d["shift"], 1)
    if pool:
        want = want.view(B * M, 64, c.N).max(dim=1)[0]
    torch.testing.assert_close(y, want, rtol=1e-12, atol=1e-12)


def _interp_loop(sparse, idx, dist2, eps):
    B, Nd = idx.shape[:2]
    out = torch.zeros(B * Nd, sparse.shape[2], dtype=torch.float64)
    e = ref.eps32(eps)
    for b in range(B):
        for n in range(Nd):
            inv = [1.0 / max(float(dist2[b, n, k]), e) for k in range(3)]
            for k in range(3):
                out[b * Nd + n] += inv[k] / sum(inv) * sparse[b, int(idx[b, n, k])].double()
    return out


@pytest.mark.parametrize("dense", ["none", "view", "cfirst"])
def test_interp_concat_equals_an_explicit_loop(dense):
    c = cases.Ic("tiny", 2, 3, 4, 5, 0 if dense == "none" else 3, 12, 1, dense, ("zero_one", "zero_all", "dup"))
    d = ref.ic_inputs(c, False, 6, CPU)
    assert float(d["dist2"].view(-1, 3)[-2].abs().max()) == 0.0 and int((d["dist2"].view(-1, 3)[-1] == 0).sum()) == 1
    assert len(set(d["idx"].view(-1, 3)[-3].tolist())) == 1
    y, tol, _ = ref.interp_concat(d["sparse"], d["idx"], d["dist2"], d["eps"], d["dense"], c.Cout)
    want = torch.zeros(c.B * c.Nd, c.Cout, dtype=torch.float64)
    want[:, :c.Cs] = _interp_loop(d["sparse"], d["idx"], d["dist2"], d["eps"])
    if c.Cd:
        want[:, c.Cs:c.Cs + c.Cd] = d["dense"].reshape(-1, c.Cd).double()
    torch.testing.assert_close(y, want, rtol=1e-12, atol=1e-14)
    assert bool((tol[:, :c.Cs] > 0).all()) and float(tol[:, c.Cs:].abs().max()) == 0.0


@pytest.mark.parametrize("yd,Cds,relu", [(0, 0, 0), (1, 0, 1), (0, 3, 1), (1, 4, 0)])
def test_interp_affine_equals_an_explicit_loop(yd, Cds, relu):
    c = cases.Ia("tiny", 2, 3, 4, 8, yd, Cds, relu, ("zero_one", "zero_all", "dup"))
    d = ref.ia_inputs(c, False, 7, CPU)
    y, tol, _ = ref.interp_affine(d["ys"], d["idx"], d["dist2"], d["eps"], d["yd"], d["dense_small"], d["wd4"], d["scale"],
                                  d["shift"], relu)
    x = _interp_loop(d["ys"], d["idx"], d["dist2"], d["eps"])
    if yd:
        assert bool(torch.isnan(d["yd"][:, c.C:]).all())
        x = x + d["yd"][:, :c.C].double()
    if Cds:
        assert Cds == 4 or float(d["wd4"][:, Cds:].abs().max()) == 0.0
        for p in range(c.B * c.Nd):
            for n in range(c.C):
                for k in range(Cds):
                    x[p, n] += float(d["wd4"][n, k]) * float(d["dense_small"][p // c.Nd, p % c.Nd, k])
    want = _module_layer(x, torch.eye(c.C), d["scale"], d["shift"], relu)
    torch.testing.assert_close(y, want, rtol=1e-12, atol=1e-13)
    assert bool((tol > 0).all()) and bool(torch.isfinite(tol).all())


def test_score_head_equals_torch_modules():
    c = cases.Sh("tiny", 7, 70)
    d = ref.sh_inputs(c, cases.SH_SPECIAL, 8, CPU)
    score, tol, (v, tol_v) = ref.score_head(d["x"], c.C, d["w"], ref.SH_BIAS, ref.SH_SCALE, ref.SH_SHIFT)
    conv = torch.nn.Conv1d(c.C, 1, 1, bias=True).double()
    bn = torch.nn.BatchNorm1d(1).double().eval()
    with torch.no_grad():
        conv.weight.copy_(d["w"].double().view(1, c.C, 1))
        conv.bias.fill_(ref.SH_BIAS)
        bn.running_mean.zero_()
        bn.running_var.fill_(1.0 - bn.eps)
        bn.weight.fill_(ref.SH_SCALE)
        bn.bias.fill_(ref.SH_SHIFT)
        want = torch.sigmoid(bn(conv(d["x"][:, :c.C].double().t().unsqueeze(0)))).view(-1)
    torch.testing.assert_close(score, want, rtol=1e-12, atol=1e-15)
    rows = d["rows"]
    assert sorted(rows) == sorted(cases.SH_SPECIAL) and 0 not in rows.values()
    assert float(v[rows["v_zero"]]) == 0.0 and float(score[rows["v_zero"]]) == 0.5
    assert 99 < float(v[rows["v_plus_100"]]) < 101 and -101 < float(v[rows["v_minus_100"]]) < -99
    assert bool((tol > 0).all()) and bool(torch.isfinite(tol).all()) and bool((tol_v > 0).all())
    assert bool(torch.isnan(d["x"][:, c.C:]).all())


# ---- exact-mode inputs are exact, bounds are usable -------------------------------------------------------------------------
def _assert_exact(parts, what):
    """Every intermediate a multiple of 2^-2 below 2^22: sums of such values are exact in fp32 in any order."""
    for i, t in enumerate(parts):
        t = t.double()
        assert bool((t * 4 == torch.round(t * 4)).all()), "%s: intermediate %d is not a multiple of 1/4" % (what, i)
        assert float(t.abs().max()) < 2 ** 22, "%s: intermediate %d reaches %g" % (what, i, float(t.abs().max()))


def _assert_bound(tol, what, positive=None):
    assert bool(torch.isfinite(tol).all()) and bool((tol >= 0).all()), what
    assert bool(((tol if positive is None else positive) > 0).all()), what


@pytest.mark.parametrize("c", cases.SA_CASES, ids=[c.id for c in cases.SA_CASES])
def test_sa_case_exact_inputs_and_bounds(c):
    Kpad = cases.sa_kpad(c)
    for relu in (0, 1):
        d = ref.sa_inputs(c, True, 11, CPU)
        y, _, parts = ref.sa_reference(c, d, relu, Kpad)
        _assert_exact(parts + [y], c.id)
        assert tuple(y.shape) == (cases.sa_rows(c) // 64 if c.pool else cases.sa_rows(c), c.N)
    d = ref.sa_inputs(c, False, 12, CPU)
    _assert_bound(ref.sa_reference(c, d, c.relu, Kpad)[1], c.id)
    tags = cases.sa_tags(c)
    if "index_extremes" in tags:
        assert {0, c.Nsrc - 1} <= set(d["nbr"].reshape(-1).tolist())
        assert c.mode == 3 or {0, c.Nsrc - 1} <= set(d["ctr"].reshape(-1).tolist())
        assert bool((d["nbr"][:, :, -1] == d["nbr"][:, :, 0]).any())
    if "row0_redirect" in tags:
        assert int(d["nbr"].reshape(-1)[0]) == c.Nsrc - 1
    if c.mode == 1 and c.Cf:
        f = d["feat"]
        vec = f.stride(2) == 1 and c.Cf % 4 == 0 and f.data_ptr() % 16 == 0 and f.stride(0) % 4 == 0 and f.stride(1) % 4 == 0
        assert vec == any(t.startswith("vec_feat") for t in tags), c.id   # the launcher's own condition for float4 loads
        if "scalar_feat_offset" in tags:
            assert f.stride(2) == 1 and f.data_ptr() % 16 == 4
        if "scalar_feat_cfirst" in tags:
            assert f.stride(2) != 1 or c.Nsrc == 1


@pytest.mark.parametrize("c", cases.IC_CASES, ids=[c.id for c in cases.IC_CASES])
def test_interp_concat_case_exact_inputs_and_bounds(c):
    d = ref.ic_inputs(c, True, 13, CPU)
    y, _, parts = ref.interp_concat(d["sparse"], d["idx"], d["dist2"], d["eps"], d["dense"], c.Cout)
    _assert_exact(parts + [y], c.id)
    assert sorted(set(parts[0].reshape(-1).tolist())) == [0.25, 0.5]
    d = ref.ic_inputs(c, False, 14, CPU)
    tol = ref.interp_concat(d["sparse"], d["idx"], d["dist2"], d["eps"], d["dense"], c.Cout)[1]
    _assert_bound(tol, c.id, tol[:, :c.Cs])
    if "dense_view" in cases.ic_tags(c):
        assert d["dense"].stride(1) == c.Cd + 3 and d["dense"].stride(2) == 1


@pytest.mark.parametrize("c", cases.IA_CASES, ids=[c.id for c in cases.IA_CASES])
def test_interp_affine_case_exact_inputs_and_bounds(c):
    for relu in (0, 1):
        d = ref.ia_inputs(c, True, 15, CPU)
        y, _, parts = ref.interp_affine(d["ys"], d["idx"], d["dist2"], d["eps"], d["yd"], d["dense_small"], d["wd4"], d["scale"],
                                        d["shift"], relu)
        _assert_exact(parts + [y], c.id)
    d = ref.ia_inputs(c, False, 16, CPU)
    _assert_bound(ref.interp_affine(d["ys"], d["idx"], d["dist2"], d["eps"], d["yd"], d["dense_small"], d["wd4"], d["scale"],
                                    d["shift"], c.relu)[1], c.id)
    if c.Cds:
        assert d["dense_small"].stride(1) == 8 and d["dense_small"].stride(2) == 1


@pytest.mark.parametrize("c", cases.SH_CASES, ids=[c.id for c in cases.SH_CASES])
def test_score_head_case_bounds(c):
    d = ref.sh_inputs(c, cases.SH_SPECIAL, 17, CPU)
    score, tol, _ = ref.score_head(d["x"], c.C, d["w"], ref.SH_BIAS, ref.SH_SCALE, ref.SH_SHIFT)
    _assert_bound(tol, c.id)
    assert set(d["rows"]) == cases.sh_tags(c) & set(cases.SH_SPECIAL)
    if "v_zero" in d["rows"]:
        assert float(score[d["rows"]["v_zero"]]) == 0.5
