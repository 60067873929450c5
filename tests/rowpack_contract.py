"""The contract of sa_chain3's row-packing plan (``fused.chain3_pair_order`` / ``regnet_pair_order_i64``), stated without the
plan's own code: used by the CPU test of the host fallback and by the GPU test of the kernel."""
import numpy as np


def parts(count):
    """Member counts -> (full 32-row point tiles, remainder rows 1..32); 32 and 64 count as a full last tile."""
    c = np.clip(np.asarray(count, dtype=np.int64).reshape(-1), 1, 64) - 1
    return c >> 5, (c & 31) + 1


def pair_cost(count, i, j):
    """Point tiles executed for neighbourhoods i and j at waves w and w + 4: one shared tile if the remainders fit 32 rows."""
    ft, rem = parts(count)
    return ft[i] + ft[j] + np.where(rem[i] + rem[j] <= 32, 1, 2)


def greedy_tiles(count):
    """Tiles of the smallest-with-largest matching of the remainders (two-pointer over the sorted remainders)."""
    ft, rem = parts(count)
    r = np.sort(rem)
    i, j, tiles = 0, len(r) - 1, 0
    while i <= j:
        if i < j and r[i] + r[j] <= 32:
            i += 1
        j -= 1
        tiles += 1
    return int(ft.sum()) + tiles


def check_plan(count, order):
    """``order`` is a permutation; slots 8 g + w and 8 g + w + 4 hold the partners; the pairs' costs ascend; the plan executes
    exactly the tiles of the greedy matching.  -> (tiles executed with whole workgroups at their heaviest pair's pace, tiles of
    the plan, tiles without any skipping)."""
    count = np.asarray(count, dtype=np.int64).reshape(-1)
    order = np.asarray(order, dtype=np.int64).reshape(-1)
    n = count.size
    assert order.shape == (n,)
    assert np.array_equal(np.sort(order), np.arange(n)), "not a permutation"
    full = n // 8
    blocks = order[:8 * full].reshape(full, 8)
    cost = pair_cost(count, blocks[:, :4], blocks[:, 4:])            # (workgroup, SIMD pair)
    flat = cost.reshape(-1)
    assert np.all(flat[1:] >= flat[:-1]), "pair costs do not ascend"
    tail = order[8 * full:]                                          # a partial last workgroup: pairs one after the other
    tail_cost = pair_cost(count, tail[0:len(tail) - 1:2], tail[1::2])
    assert np.all(tail_cost >= (flat[-1] if flat.size else 0))
    ft, _ = parts(count)
    single = int(ft[tail[-1]]) + 1 if n % 2 else 0
    tiles = int(flat.sum()) + int(tail_cost.sum()) + single
    assert tiles == greedy_tiles(count), (tiles, greedy_tiles(count))
    paced = int(cost.max(axis=1).sum()) * 4 + int(tail_cost.sum()) + single if full else tiles
    return paced, tiles, 2 * n


def count_cases(n, seed):
    """Count distributions for a plan of n neighbourhoods: uniform, all full, all tiny, bench-like (many full, many half)."""
    rng = np.random.default_rng(seed)
    yield rng.integers(1, 65, n)
    yield np.full(n, 64)
    yield rng.integers(1, 17, n)
    yield np.minimum(64, rng.integers(1, 120, n))
    yield rng.choice([1, 15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64], n)
    yield rng.integers(17, 33, n)          # no two remainders fit
