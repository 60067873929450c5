"""Pins tests/f64_reference.py (the float64 restatement the GPU's float64 kernels are compared with) against the float32
C oracle, independently of any GPU: on integer-lattice clouds scaled by a power of two every coordinate, difference,
square and sum is exact in both precisions, so the two must pick the same indices bit for bit -- duplicates, ties, zero
extent, sizes that are not powers of two and clouds below the reference's 16-lane minimum included."""
import numpy as np
import pytest
import torch

from oracle import pn2_ext_oracle as O

from . import f64_reference as R

SCALE = 2.0 ** -5


def lattice(seed, B, N, span, dup=0.0):
    """(B, 3, N) float64 cloud on the lattice SCALE * Z^3 with coordinates in [0, span); ``dup``: share of points that
    repeat an earlier one."""
    rng = np.random.default_rng(seed)
    p = rng.integers(0, span, size=(B, N, 3)).astype(np.float64)
    if dup > 0 and N > 1:
        rep = rng.random((B, N)) < dup
        src = rng.integers(0, N, size=(B, N))
        for b in range(B):
            for j in np.nonzero(rep[b])[0]:
                p[b, j] = p[b, min(src[b, j], j)]
    return torch.from_numpy(p * SCALE).transpose(1, 2).contiguous()


CLOUDS = [  # (seed, B, N, span, dup)
    (1, 2, 1000, 40, 0.0),      # N not a power of two
    (2, 2, 1024, 6, 0.3),       # dense lattice: many equal distances, duplicates
    (3, 1, 777, 3, 0.5),        # very coarse: ties everywhere
    (4, 2, 12, 5, 0.2),         # N < 16: the reference still runs 16 lanes
    (5, 1, 3000, 64, 0.0),      # block 512, several points per lane
]


@pytest.mark.parametrize("seed,B,N,span,dup", CLOUDS)
def test_fps_matches_oracle_on_lattices(seed, B, N, span, dup):
    x = lattice(seed, B, N, span, dup)
    M = min(N, 300)
    got = R.farthest_point_sample(x, M)
    want = O.farthest_point_sample(x.float(), M)
    assert torch.equal(got, want)


def test_fps_zero_extent_repeats_the_previous_pick():
    x = torch.full((2, 3, 50), 0.75, dtype=torch.float64)
    got = R.farthest_point_sample(x, 20)
    assert torch.equal(got, O.farthest_point_sample(x.float(), 20))
    assert torch.equal(got, torch.zeros(2, 20, dtype=torch.int64))
    # two distinct points: after both are picked every distance is 0 and the last pick repeats
    y = torch.zeros(1, 3, 17, dtype=torch.float64)
    y[0, 0, 9] = 1.0
    got = R.farthest_point_sample(y, 5)
    assert torch.equal(got, O.farthest_point_sample(y.float(), 5))


@pytest.mark.parametrize("seed,B,N,span,dup", CLOUDS)
@pytest.mark.parametrize("radius_steps,K", [(5, 16), (9, 64), (1, 4)])
def test_ball_query_matches_oracle_on_lattices(seed, B, N, span, dup, radius_steps, K):
    x = lattice(seed, B, N, span, dup)
    c = x[:, :, ::3].contiguous()
    radius = radius_steps * SCALE      # exact in float32: d2 == r2 boundaries are hit and must stay outside (strict <)
    gi, gc = R.ball_query(x, c, radius, K)
    wi, wc = O.ball_query(x.float(), c.float(), radius, K)
    assert torch.equal(gi, wi) and torch.equal(gc, wc)


def test_ball_query_radius_rounds_to_float32():
    # 0.1 is not a float32: the reference squares float(0.1) (ball_query_kernel.cu:90); a point between the float32
    # and the float64 radius tells the two apart
    r32 = float(np.float32(0.1))
    assert r32 > 0.1
    d = (0.1 + r32) / 2.0
    x = torch.tensor([[[0.0, d, 0.5], [0.0, 0.0, 0.0], [0.0, 0.0, 0.0]]], dtype=torch.float64)
    c = x[:, :, :1].contiguous()
    idx, cnt = R.ball_query(x, c, 0.1, 4)
    assert cnt.tolist() == [[2]] and idx.tolist() == [[[0, 1, 0, 0]]]


def test_ball_query_empty_ball_keeps_zeros():
    x = torch.zeros(1, 3, 8, dtype=torch.float64)
    c = torch.full((1, 3, 2), 5.0, dtype=torch.float64)
    idx, cnt = R.ball_query(x, c, 0.5, 3)
    assert torch.equal(idx, torch.zeros(1, 2, 3, dtype=torch.int64)) and torch.equal(cnt, torch.zeros(1, 2, dtype=torch.int64))


@pytest.mark.parametrize("seed,B,N,span,dup", CLOUDS)
def test_three_nn_matches_oracle_on_lattices(seed, B, N, span, dup):
    x = lattice(seed, B, N, span, dup)
    keys = x[:, :, : max(3, N // 4)].contiguous()
    gi, gd = R.point_search(x, keys, 3)
    wi, wd = O.point_search(x.float(), keys.float(), 3)
    assert torch.equal(gi, wi)
    assert torch.equal(gd.float(), wd) and torch.equal(gd.float().double(), gd)   # exact squared distances


def test_backward_sums_in_source_order():
    # contributions chosen so that the float64 sum depends on its order: ascending source position from +0.0
    g = torch.tensor([1.0, 1e-16, -1.0, 1e-16], dtype=torch.float64).view(1, 1, 2, 2)
    idx = torch.zeros(1, 2, 2, dtype=torch.int64)
    got = R.group_points_backward(g, idx, 3)
    want = ((0.0 + 1.0) + 1e-16) + -1.0
    want = want + 1e-16
    assert got[0, 0, 0].item() == want and got[0, 0, 1].item() == 0.0
    assert not np.signbit(got[0, 0, 2].item())
    # interpolate: the rounded products g * w, position n * 3 + k
    gi = R.interpolate_backward(torch.tensor([[[3.0, 5.0]]], dtype=torch.float64), torch.tensor([[[1, 1, 0], [1, 0, 0]]]),
                                torch.tensor([[[0.1, 0.2, 0.7], [0.3, 0.3, 0.4]]], dtype=torch.float64), 2)
    assert gi[0, 0, 1].item() == ((0.0 + 3.0 * 0.1) + 3.0 * 0.2) + 5.0 * 0.3
    assert gi[0, 0, 0].item() == ((0.0 + 3.0 * 0.7) + 5.0 * 0.3) + 5.0 * 0.4


def test_forward_gathers():
    x = torch.arange(12, dtype=torch.float64).view(1, 2, 6)
    idx = torch.tensor([[[5, 0], [2, 2]]])
    out = R.group_points_forward(x, idx)
    assert out.tolist() == [[[[5.0, 0.0], [2.0, 2.0]], [[11.0, 6.0], [8.0, 8.0]]]]
    w = torch.tensor([[[0.5, 0.25, 0.25]]], dtype=torch.float64)
    y = R.interpolate_forward(x, torch.tensor([[[1, 3, 5]]]), w)
    assert y[0, 0, 0].item() == ((0.0 + 1.0 * 0.5) + 3.0 * 0.25) + 5.0 * 0.25
