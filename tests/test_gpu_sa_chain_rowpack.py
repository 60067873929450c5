"""sa_chain3's row packing (csrc/sa_chain.hip: two neighbourhoods at waves w and w + 4 share a point tile at their true row
split) and its plan (csrc/gather.hip: pair_order_kernel).  The packing is exact: every call with ``count`` must return the bits
of the call without it, under the plan's order, without an order and under any other permutation."""
import numpy as np
import pytest
import torch

from tests import rowpack_contract as C

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
G = 64
EVERY = [1, 15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64]


def _layer(N, K, relu, seed, order=None):
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
    return fused._pack(conv.to(DEV), bn.to(DEV).eval(), relu, order)


def _block(count, C3, Cf, relu3, seed):
    """Random scene, neighbour table padded ball-query style (slots behind ``count`` repeat slot 0), packed layers."""
    B, M = count.shape
    N = 700
    rng = np.random.default_rng(seed)
    pc = torch.from_numpy(rng.normal(size=(B, N, 3 + max(Cf, 1))).astype(np.float32)).to(DEV)
    xyz = pc[:, :, :3].permute(0, 2, 1)
    feat = pc[:, :, 3:3 + Cf].permute(0, 2, 1) if Cf else None
    nbr = torch.from_numpy(rng.integers(0, N, (B, M, G))).to(DEV)
    ctr = torch.from_numpy(rng.integers(0, N, (B, M))).to(DEV)
    count = torch.as_tensor(count, dtype=torch.int64).to(DEV)
    slot = torch.arange(G, device=DEV).view(1, 1, G)
    nbr = torch.where(slot < count.unsqueeze(-1), nbr, nbr[:, :, :1].expand(B, M, G)).contiguous()
    cols = torch.cat([torch.arange(3, 3 + Cf), torch.arange(3)]).to(DEV)
    layers = (_layer(128, Cf + 3, True, seed + 1, cols), _layer(128, 128, True, seed + 2), _layer(C3, 128, relu3, seed + 3))
    return feat, xyz, nbr, ctr, layers, count


def _check_exact(count, C3, Cf, relu3=True, seed=7, orders=()):
    from regnet_for_3d_grasping_amd import fused
    count = np.asarray(count, dtype=np.int64)
    B, M = count.shape
    feat, xyz, nbr, ctr, (l1, l2, l3), cnt = _block(count, C3, Cf, relu3, seed)
    plain = fused.sa_chain3(feat, xyz, nbr, ctr, l1, l2, l3, B, M, G)
    assert bool(torch.isfinite(plain).all())
    if not relu3 and count.min() == 1:   # (a single member: its channels' maxima are its own values, about half below 0)
        assert bool((plain < 0).any())          # a selected maximum that started from 0 would show here
    rng = np.random.default_rng(seed)
    plan = fused.chain3_pair_order(cnt)
    C.check_plan(count, plan.cpu().numpy())
    named = [("plan", plan), ("none", None), ("three classes", fused.chain3_order(cnt)),
             ("random", torch.from_numpy(rng.permutation(B * M)).to(DEV)), ("reversed plan", plan.flip(0))]
    named += [(str(i), torch.as_tensor(o, dtype=torch.int64).to(DEV)) for i, o in enumerate(orders)]
    for name, order in named:
        got = fused.sa_chain3(feat, xyz, nbr, ctr, l1, l2, l3, B, M, G, cnt, order)
        assert torch.equal(got, plain), "order '%s': %d of %d values differ" % (name, int((got != plain).sum()), got.numel())


# (host count, guest count) at slots w and w + 4, written down pair by pair: remainder sums of exactly 32 and 33, a guest that
# fits whole (both <= 32), hosts with one and two tiles, the old fixed split (48, 48), full ones, and every count of EVERY
PAIRS = [(1, 31), (15, 17), (16, 16), (17, 15),        # sums of 32: the guest has no tile of its own
         (32, 1), (31, 33), (47, 48), (48, 47),        # 32 + 1 = 33 rows: no sharing; a 33 whose single row moves; 15 + 16
         (49, 15), (63, 1), (64, 1), (48, 48),         # 17 + 15, 31 + 1 share; 32 + 1 does not; the split at 16
         (47, 49), (33, 63), (64, 64), (2, 30),        # two full tiles + 15 + 17; 1 + 31; nothing to share; 2 + 30
         (1, 32), (17, 16), (16, 17), (33, 33),        # 33 rows again; 33 rows; 33 rows; 1 + 1
         (1, 1), (31, 1), (49, 48), (63, 33)]          # two rows in one tile; ...; 17 + 16 = 33 rows; 31 + 1


def _pairs_as_slots(pairs):
    """Pairs -> counts in slot order (four pairs per workgroup: hosts at w, guests at w + 4)."""
    out = []
    for g in range(0, len(pairs), 4):
        out += [p[0] for p in pairs[g:g + 4]] + [p[1] for p in pairs[g:g + 4]]
    return out


@pytest.mark.parametrize("C3,Cf,relu3", [(256, 3, True), (64, 0, True), (160, 5, True), (64, 3, False)])
def test_written_down_pairs_are_bit_identical(C3, Cf, relu3):
    """Every case of PAIRS at waves w, w + 4 as the slots come (no order), mirrored (guest left, host right), and the same
    neighbourhoods under the plan and other permutations; the 48 slots are two scenes of 24, so workgroups 2 and 3 pair across
    the scene boundary."""
    slots = _pairs_as_slots(PAIRS)
    assert set(EVERY) <= set(slots)
    mirrored = _pairs_as_slots([(b, a) for a, b in PAIRS])
    for s in (slots, mirrored):
        _check_exact(np.array(s).reshape(2, 24), C3, Cf, relu3, seed=11)


@pytest.mark.parametrize("B,M,C3,Cf,relu3", [(3, 37, 256, 3, True), (1, 13, 160, 5, True), (2, 25, 64, 0, False),
                                             (5, 7, 256, 3, True), (1, 1, 64, 3, True), (1, 4, 64, 3, True), (1, 5, 64, 3, True)])
def test_random_counts_odd_sizes_are_bit_identical(B, M, C3, Cf, relu3):
    """B M not a multiple of 8 (invalid trailing waves, partners beyond the end), odd numbers of candidates (one left
    unpaired), partners from different scenes; counts uniform, from EVERY, and all small (everything pairs, guests fit whole)."""
    rng = np.random.default_rng(B * 100 + M)
    for count in (rng.integers(1, G + 1, (B, M)), rng.choice(EVERY, (B, M)), rng.integers(1, 17, (B, M))):
        _check_exact(count, C3, Cf, relu3, seed=B + M)


def test_pipeline_shape_is_bit_identical():
    """One scene batch of the forward's level-1 shape in small (2 x 1024 neighbourhoods, counts spread like a synthetic scene's),
    under the plan: whole workgroups of every cost class."""
    rng = np.random.default_rng(3)
    count = np.clip(rng.normal(41, 18, (2, 1024)).round().astype(np.int64), 1, 64)
    _check_exact(count, 256, 3, True, seed=5)


@pytest.mark.parametrize("n", [1, 2, 7, 8, 9, 63, 65, 1024, 1025, 40960, 8 * 5120 + 3, 100001])
def test_plan_kernel_keeps_the_contract_and_equals_the_host_plan(n):
    from regnet_for_3d_grasping_amd import fused, pn2_ext
    for count in C.count_cases(n, n):
        c = torch.from_numpy(count.astype(np.int64)).to(DEV)
        order = pn2_ext.pair_order(c)
        assert order.dtype == torch.int64 and tuple(order.shape) == (n,)
        got = order.cpu().numpy()
        C.check_plan(count, got)
        assert np.array_equal(got, fused.chain3_pair_order(c.cpu()).numpy())      # the numpy restatement, run for run
        assert torch.equal(fused.chain3_pair_order(c.view(1, -1)), order)        # deterministic
    out_of_range = torch.tensor([0, -3, 65, 1000, 5, 64, 33, 2, 40], device=DEV)    # clamped to 1..64 like the chain kernel does
    C.check_plan(out_of_range.cpu().numpy(), pn2_ext.pair_order(out_of_range).cpu().numpy())
