"""csrc/outlier.hip on the device against the numpy restatement (tests/outlier_reference.py): ``count``, ``found``, the bits of
``mean_dist``, ``status``, ``num`` and ``keep`` of every case, each run twice for equal bytes.  The statistics are held against
``math.fsum`` within the bound of any summation order, and ``keep`` exactly against the device's own threshold."""
import ctypes
import math

import numpy as np
import pytest
import torch

from . import outlier_reference as ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
f32 = np.float32
UNIT = 2.0 ** -13          # coordinates on this lattice below 1 m: every difference, product and sum of a d2 is exact in float32


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _bytes(t):
    return None if t is None else t.cpu().numpy().tobytes()


def _check(xyz, mask=None, device_xyz=None, **params):
    """``filter_cloud`` twice on the device and once in numpy -> (device result, restatement)."""
    from regnet_for_3d_grasping_amd import outliers
    p = outliers.OutlierParams(**params)
    x = _dev(xyz) if device_xyz is None else device_xyz
    m = None if mask is None else _dev(np.asarray(mask))
    got, again = outliers.filter_cloud(x, p, m), outliers.filter_cloud(x, p, m)
    for name in ("keep", "status", "num", "stats", "mean_dist", "count", "found"):
        assert _bytes(getattr(got, name)) == _bytes(getattr(again, name)), name
    thr = None if got.stats is None else got.stats.cpu().numpy()[3]
    want = ref.filter_cloud(xyz, p.mode, p.radius, p.min_neighbours, p.knn, p.max_radius, p.std_ratio, mask=mask, thr=thr)
    for name in ("count", "found"):
        if want[name] is not None:
            value = getattr(got, name)
            assert value.dtype == torch.int32 and np.array_equal(value.cpu().numpy(), want[name]), name
    if want["mean_dist"] is not None:
        assert got.mean_dist.dtype == torch.float32
        assert np.array_equal(got.mean_dist.cpu().numpy().view(np.uint32), want["mean_dist"].view(np.uint32))
        _check_stats(got.stats.cpu().numpy(), want["mean_dist"], want["found"], p.knn, p.std_ratio)
    assert got.status.dtype == torch.uint8 and got.keep.dtype == torch.bool and got.num.dtype == torch.int32
    assert np.array_equal(got.status.cpu().numpy(), want["status"])        # (keep: exact against the device's own threshold)
    assert np.array_equal(got.keep.cpu().numpy(), want["keep"]) and np.array_equal(got.num.cpu().numpy(), want["num"])
    assert got.counts() == tuple(int(v) for v in want["num"])
    return got, want


def _check_stats(stats, mean, found, k, ratio):
    """n exact; mu and sigma within the bound of any float64 summation order against ``math.fsum``; thr from the device's own
    mu and sigma, exactly.

    The bounds: a sum of n terms in any order errs by at most n 2^-53 sum|x| (``ref.sum_bound``); mu adds the division's
    rounding.  sigma = ||m - mu|| / sqrt(n - 1) moves by at most sqrt(n / (n - 1)) <= sqrt 2 times a change of mu, its n
    non-negative terms carry two roundings each and the sum n more (relative (n + 4) 2^-53 on the sum of squares, half of it
    on the root), and the division and the root round once each."""
    n, mu, sigma, thr = ref.stats(mean, found, k, ratio)
    m = mean[found == k].astype(np.float64)
    assert stats[0] == n
    if n == 0:
        assert math.isnan(stats[1]) and math.isnan(stats[2]) and stats[3] == math.inf
        return
    d_mu = ref.sum_bound(m) / n + 2.0 ** -53 * abs(mu)
    assert abs(stats[1] - mu) <= d_mu
    if n == 1:
        assert math.isnan(stats[2]) and stats[3] == math.inf
        return
    assert abs(stats[2] - sigma) <= sigma * ((n + 4) * 2.0 ** -54 + 2.0 ** -52) + math.sqrt(2.0) * d_mu
    assert stats[3] == float(f32(stats[1] + float(ratio) * stats[2]))


def _cloud(n, seed, extent=0.1):
    return np.random.RandomState(seed).uniform(0.0, extent, size=(n, 3)).astype(np.float32)


# ---- thresholds -------------------------------------------------------------------------------------------------------------------
def _three_squares(total, lo=2900):
    """Integers (a, b, c), a >= lo, with a^2 + b^2 + c^2 == total."""
    for a in range(math.isqrt(total), lo, -1):
        for b in range(0, 1200):
            c2 = total - a * a - b * b
            if c2 < 0:
                break
            c = math.isqrt(c2)
            if c * c == c2:
                return a, b, c
    raise AssertionError("no representation")


def _threshold_cloud():
    """-> (pts, R): a centre and three partners at d2 == R2, one ulp below and one ulp above, all coordinates exactly
    representable, every partner more than R from the others.  R is the first float32 from 0.375 up in steps of 2^-12 whose R2 =
    M units^2 (its ulp is one unit^2) has M = 2 mod 8, so that M - 1, M and M + 1 are all sums of three squares."""
    for j in range(64):
        R = f32(0.375 + j * 2.0 ** -12)
        M = int(float(R * R) * 2.0 ** 26)
        if M % 8 == 2 and float(R * R) * 2.0 ** 26 == M:
            break
    centre = np.array([[0.5, 0.5, 0.5]])
    at, below, above = (np.array(_three_squares(t), dtype=np.float64) * UNIT for t in (M, M - 1, M + 1))
    pts = np.concatenate([centre, centre + at, centre + below[[1, 0, 2]] * [1, -1, 1], centre - above[[2, 1, 0]]]).astype(np.float32)
    d2 = ref.d2_block(pts[:1], pts[1:])[0]
    R2 = R * R
    assert d2.tolist() == [R2, np.nextafter(R2, f32(0)), np.nextafter(R2, f32(np.inf))]
    assert (ref.d2_block(pts[1:], pts[1:])[~np.eye(3, dtype=bool)] > R2 * f32(1.5)).all()
    return pts, float(R)


def test_the_radius_threshold_at_one_ulp():
    pts, R = _threshold_cloud()
    got, _ = _check(pts, mode="radius", radius=R, min_neighbours=3)
    assert got.count.cpu().tolist() == [2, 1, 1, 0]
    got, _ = _check(pts, mode="statistical", knn=2, max_radius=R, std_ratio=0.0)
    assert got.found.cpu().tolist() == [2, 1, 1, 0]
    assert got.stats.cpu()[0] == 1.0 and got.keep.cpu().tolist() == [True, False, False, False]


# ---- the radius count -------------------------------------------------------------------------------------------------------------
def _ring(centre, n, r=0.03):
    a = np.linspace(0, 2 * math.pi, n, endpoint=False)
    return np.asarray(centre) + np.stack([r * np.cos(a), r * np.sin(a), np.zeros(n)], axis=1)


def test_one_fewer_exactly_and_far_more_than_min_neighbours():
    rng = np.random.RandomState(1)
    parts = [np.array([[0.0, 0, 0]]), _ring((0, 0, 0), 15), np.array([[1.0, 0, 0]]), _ring((1, 0, 0), 16),
             np.array([2.0, 0, 0]) + 0.004 * rng.standard_normal((100, 3)),          # > 64 rows in one cell
             np.array([3.0, 0, 0]) + 0.004 * rng.standard_normal((300, 3))]          # > 256
    pts = np.concatenate(parts).astype(np.float32)
    got, want = _check(pts, mode="radius")
    count = got.count.cpu().numpy()
    assert count[0] == 15 and count[16] == 16 and (count[33:] == 16).all()
    assert not got.keep[0] and got.keep[16]
    _check(pts, mode="radius", min_neighbours=299)
    big = _check(pts, mode="radius", min_neighbours=10 ** 6)[0].count.cpu().numpy()
    assert big[133:].tolist() == [299] * 300 and big[33:133].tolist() == [99] * 100
    _check(pts, mode="both", knn=15)


def test_the_row_itself_a_duplicate_and_all_rows_identical():
    same = np.full((130, 3), 0.125, dtype=np.float32)
    got, _ = _check(same, mode="radius", radius=0.01, min_neighbours=200)
    assert got.count.cpu().tolist() == [129] * 130
    got, _ = _check(same, mode="statistical", knn=64, max_radius=0.01)
    assert got.found.cpu().tolist() == [64] * 130 and got.mean_dist.cpu().tolist() == [0.0] * 130 and got.keep.all()
    pts = _cloud(100, 2)
    pts[10] = pts[90]
    got, _ = _check(pts, mode="radius", radius=1e-4, min_neighbours=2)
    assert got.count.cpu()[[10, 90]].tolist() == [1, 1] and int(got.count.sum()) == 2


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
@pytest.mark.parametrize("mode", ["radius", "statistical", "both"])
def test_row_counts_around_a_wave(n, mode):
    _check(_cloud(n, n), mode=mode, radius=0.03, min_neighbours=5, knn=4, max_radius=0.03)


def test_faces_of_the_box_a_coarsened_grid_and_the_last_cells():
    lattice = (np.stack(np.meshgrid(*[np.arange(9)] * 3, indexing="ij"), axis=-1).reshape(-1, 3) / 64.0).astype(np.float32)
    got, _ = _check(lattice, mode="radius", radius=1.0 / 64, min_neighbours=6)          # every border row sits on a face of the box
    assert int(got.keep.sum()) == 7 ** 3
    _check(lattice, mode="statistical", knn=6, max_radius=0.0157)
    _check(lattice, mode="radius", radius=0.5, min_neighbours=700)                  # one cell; the ball reaches outside the grid
    far = np.concatenate([_cloud(400, 3), [[64.0, 0.05, 0.05]], [[-64.0, 64.0, 0.05]]]).astype(np.float32)
    _check(far, mode="radius", radius=0.02, min_neighbours=8)                        # 128 m / 0.02 m: the grid coarsens
    _check(far, mode="both", radius=0.02, min_neighbours=8, knn=8, max_radius=0.02)


def test_nan_inf_and_masked_rows_at_wave_boundaries_and_strides():
    pts = _cloud(260, 4)
    pts[[63, 64, 65], 0] = np.nan
    pts[127, 1] = np.inf
    pts[128, 2] = -np.inf
    mask = np.ones(260, dtype=bool)
    mask[[0, 191, 192, 255, 256, 259]] = False
    for mode in ("radius", "statistical", "both"):
        got, _ = _check(pts, mask, mode=mode, radius=0.03, min_neighbours=5, knn=4, max_radius=0.03)
        assert (got.status.cpu().numpy()[[0, 63, 64, 65, 127, 128, 191, 192, 255, 256, 259]] == 0).all()
    _check(pts, mask.astype(np.uint8) * 7, mode="radius", radius=0.03, min_neighbours=5)
    wide = torch.zeros((260, 7), dtype=torch.float32, device=DEV)
    wide[:, 2:5] = _dev(pts)
    _check(pts, mask, device_xyz=wide[:, 2:5], mode="both", radius=0.03, min_neighbours=5, knn=4, max_radius=0.03)
    _check(pts, device_xyz=_dev(pts.T.copy()).T, mode="radius", radius=0.03, min_neighbours=5)
    double = pts.astype(np.float64) + 1e-10                 # float64 in: decided on its float32 rounding
    _check(double.astype(np.float32), device_xyz=_dev(double), mode="both", radius=0.03, min_neighbours=5, knn=4, max_radius=0.03)


# ---- the k nearest ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 2, 63, 64])
def test_k_at_its_limits_and_one_neighbour_short(k):
    rng = np.random.RandomState(k)
    pts = np.concatenate([0.01 * rng.standard_normal((400, 3)),                     # far more than k in the ball
                          [1.0, 0, 0] + 0.005 * rng.uniform(-1, 1, (k + 1, 3)),     # found == k exactly
                          [2.0, 0, 0] + 0.005 * rng.uniform(-1, 1, (k, 3))]).astype(np.float32)     # found == k - 1
    got, _ = _check(pts, mode="statistical", knn=k, max_radius=0.03)
    found = got.found.cpu().numpy()
    assert (found[400:401 + k] == k).all() and (found[401 + k:] == k - 1).all() and (found[:400] == k).mean() > 0.5
    assert (got.status.cpu().numpy()[401 + k:] == ref.TOO_FEW_NEAREST).all()


def test_arrival_orders_runs_of_equal_distance_and_ties_at_the_kth():
    line = np.zeros((150, 3))
    line[:, 0] = np.arange(150) * 32 * UNIT                # along the cells' x-run, which the walk takes in ascending x: cell by
    _check(line.astype(np.float32), mode="statistical", knn=12, max_radius=0.05)         # cell, the first row meets its candidates
    _check(line[::-1].astype(np.float32), mode="statistical", knn=20, max_radius=0.05)   # nearest first, the last row farthest first
    _check(line.astype(np.float32), mode="statistical", knn=64, max_radius=0.3)
    # 48 rows at ONE d2 from the centre (the signed permutations of (3, 2, 1) units), 24 at another, the centre itself
    import itertools
    shell = np.array([[s0 * p[0], s1 * p[1], s2 * p[2]] for p in itertools.permutations((3, 2, 1))
                      for s0 in (1, -1) for s1 in (1, -1) for s2 in (1, -1)], dtype=np.float64)
    inner = np.array([[s0 * p[0], s1 * p[1], 0] for p in itertools.permutations((2, 1)) for s0 in (1, -1) for s1 in (1, -1)]
                     + [[s0 * p[0], 0, s1 * p[1]] for p in itertools.permutations((2, 1)) for s0 in (1, -1) for s1 in (1, -1)]
                     + [[0, s0 * p[0], s1 * p[1]] for p in itertools.permutations((2, 1)) for s0 in (1, -1) for s1 in (1, -1)], dtype=np.float64)
    pts = (0.5 + np.concatenate([[[0, 0, 0]], shell, inner]) * 64 * UNIT).astype(np.float32)
    assert len(np.unique(ref.d2_block(pts[:1], pts[1:]))) == 2
    for k in (1, 23, 24, 25, 40, 64):                      # more than k ties at the k-th value, and the k-th inside a run
        got, _ = _check(pts, mode="statistical", knn=k, max_radius=0.1)
        assert got.found.cpu()[0] == k
    got, _ = _check(pts, mode="statistical", knn=30, max_radius=float(f32(math.sqrt(14.0) * 64 * UNIT)))


def test_max_radius_at_one_ulp():
    pts, R = _threshold_cloud()
    got, _ = _check(pts, mode="statistical", knn=1, max_radius=R)
    assert got.found.cpu().tolist() == [1, 1, 1, 0]
    below = float(np.sqrt(np.nextafter(f32(R) * f32(R), f32(0))))
    assert got.mean_dist.cpu().tolist()[:3] == [below, float(np.sqrt(f32(R) * f32(R))), below]


# ---- the statistics ---------------------------------------------------------------------------------------------------------------
def test_statistics_of_no_one_and_two_rows_and_ratio_zero():
    a, b, c = [0.0, 0, 0], [0.03, 0, 0], [-0.03, 0, 0]
    got, _ = _check(np.array([a, [1.0, 0, 0]], dtype=np.float32), mode="statistical", knn=1)
    assert got.stats.cpu()[0] == 0 and got.num.cpu().tolist() == [0, 0, 2, 0, 0]
    got, _ = _check(np.array([a, b, c], dtype=np.float32), mode="statistical", knn=2)       # only a has two within 0.04
    assert got.stats.cpu()[0] == 1 and got.keep.cpu().tolist() == [True, False, False]
    got, _ = _check(np.array([a, b], dtype=np.float32), mode="statistical", knn=1)
    assert got.stats.cpu()[0] == 2 and got.keep.all()
    pts = _cloud(500, 6)
    got, _ = _check(pts, mode="statistical", knn=5, std_ratio=0.0)
    assert float(got.stats[2]) > 0 and float(got.stats[3]) == float(f32(float(got.stats[1])))
    assert 0 < int(got.keep.sum()) < 500


def test_the_two_pass_deviation_keeps_a_small_spread_on_a_large_offset():
    from regnet_for_3d_grasping_amd import outliers
    rng = np.random.RandomState(8)
    for n in (3, 1000, 5000):
        m = (1.0 + 1e-6 * rng.standard_normal(n)).astype(np.float32)
        found = np.full(n, 7, dtype=np.int32)
        found[::9] = 6                                     # rows that take no part
        stats = outliers.distance_stats(_dev(m), _dev(found), 7, 2.0).cpu().numpy()
        assert stats.tobytes() == outliers.distance_stats(_dev(m), _dev(found), 7, 2.0).cpu().numpy().tobytes()
        _check_stats(stats, m, found, 7, 2.0)
        sigma = ref.stats(m, found, 7, 2.0)[2]
        assert abs(stats[2] - sigma) <= 1e-9 * sigma       # (the one-pass form is off by 1e-6 and more here: the CPU test)


def test_both_hands_the_second_stage_only_the_survivors():
    from regnet_for_3d_grasping_amd import outliers
    rng = np.random.RandomState(5)
    cloud = np.concatenate([0.01 * rng.standard_normal((300, 3)), 0.05 * rng.standard_normal((200, 3)),
                            [[1.0, 0, 0], [1.005, 0, 0]]]).astype(np.float32)
    got, want = _check(cloud, mode="both", radius=0.02, min_neighbours=6, knn=5, max_radius=0.02, std_ratio=1.0)
    first = outliers.radius_count(_dev(cloud), None, 0.02, 6)
    survivors = first == 6
    mean, found = outliers.knn_mean_distance(_dev(cloud), survivors, 5, 0.02)
    assert _bytes(mean) == _bytes(got.mean_dist) and _bytes(found) == _bytes(got.found) and _bytes(first) == _bytes(got.count)
    assert (got.found[~survivors] == -1).all() and (got.status[~survivors] == 1).all()
    assert got.num.cpu().tolist()[1] > 0 and got.num.cpu().tolist()[3] > 0 and got.status.cpu()[-2:].tolist() == [1, 1]
    alone = _check(cloud, mode="statistical", knn=1, max_radius=0.02)[0]
    assert alone.found.cpu()[-2:].tolist() == [1, 1]


def test_apply_blanks_the_removed_rows_and_leaves_the_callers_tensors():
    pts = _cloud(300, 9)
    rgb = np.random.RandomState(9).rand(300, 3).astype(np.float32)
    got, want = _check(pts, mode="radius", radius=0.02, min_neighbours=4)
    keep = want["keep"]
    assert 0 < keep.sum() < 300
    for dtype in (np.float32, np.float64):
        x, c = _dev(pts.astype(dtype)), _dev(rgb.astype(dtype))
        x0, c0 = x.clone(), c.clone()
        ox, oc = got.apply(x, c)
        assert ox.dtype == x.dtype and oc.dtype == c.dtype and torch.equal(x, x0) and torch.equal(c, c0)
        wx, wc = ref.apply(keep, pts.astype(dtype), rgb.astype(dtype))
        assert ox.cpu().numpy().tobytes() == wx.tobytes() and oc.cpu().numpy().tobytes() == wc.tobytes()
        assert got.apply(x).cpu().numpy().tobytes() == wx.tobytes()
    assert (got.apply(_dev(pts))[~got.keep].cpu().numpy().view(np.uint32) == ref.QNAN_BITS).all()
    u8 = got.apply(_dev(pts), torch.full((300, 3), 9, dtype=torch.uint8, device=DEV))[1]
    assert u8.dtype == torch.uint8 and (u8[~got.keep] == 0).all() and (u8[got.keep] == 9).all()


# ---- the entry points -------------------------------------------------------------------------------------------------------------
def test_error_codes_precede_any_launch_and_zero_rows_touch_nothing():
    from regnet_for_3d_grasping_amd import _lib, outliers
    L = _lib.lib
    pts = _dev(_cloud(10, 1))
    sentinel = lambda dtype: torch.full((10,), 77, dtype=dtype, device=DEV)
    count, found, mean = sentinel(torch.int32), sentinel(torch.int32), sentinel(torch.float32)
    ws = torch.empty((outliers.workspace_bytes(10),), dtype=torch.uint8, device=DEV)
    stats = torch.full((4,), 77.0, dtype=torch.float64, device=DEV)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    X, C, F, M, W, S = (t.data_ptr() for t in (pts, count, found, mean, ws, stats))
    radius = lambda **kw: L.regnet_outlier_radius_f32(kw.get("x", X), None, kw.get("n", 10), kw.get("r", 0.04), kw.get("mn", 16),
                                                      kw.get("c", C), kw.get("w", W), st)
    knn = lambda **kw: L.regnet_outlier_knn_f32(kw.get("x", X), None, kw.get("n", 10), kw.get("k", 3), kw.get("r", 0.04), kw.get("m", M),
                                                kw.get("f", F), kw.get("w", W), st)
    SHAPE, NULL, UNSUPPORTED = -1, -2, -3
    assert radius(n=-1) == knn(n=-1) == L.regnet_outlier_stats_f64(M, F, -1, 3, 2.0, S, st) == SHAPE
    for bad in ({"n": 1 << 31}, {"mn": 0}, {"r": 0.0}, {"r": -1.0}, {"r": math.inf}, {"r": math.nan}):
        assert radius(**bad) == UNSUPPORTED, bad
    for bad in ({"n": 1 << 31}, {"k": 0}, {"k": 65}, {"r": 0.0}, {"r": math.inf}, {"r": math.nan}):
        assert knn(**bad) == UNSUPPORTED, bad
    assert L.regnet_outlier_stats_f64(M, F, 10, 65, 2.0, S, st) == L.regnet_outlier_stats_f64(M, F, 10, 3, -1.0, S, st) == UNSUPPORTED
    assert radius(n=-1, r=0.0, x=None) == SHAPE and radius(r=0.0, x=None) == UNSUPPORTED         # the order of the checks
    for bad in ({"x": None}, {"c": None}, {"w": None}):
        assert radius(**bad) == NULL, bad
    for bad in ({"x": None}, {"m": None}, {"f": None}, {"w": None}):
        assert knn(**bad) == NULL, bad
    assert L.regnet_outlier_stats_f64(M, F, 10, 3, 2.0, None, st) == L.regnet_outlier_stats_f64(None, F, 10, 3, 2.0, S, st) == NULL
    assert radius(n=0, x=None, c=None, w=None) == 0 and knn(n=0, x=None, m=None, f=None, w=None) == 0
    torch.cuda.synchronize()
    assert (count == 77).all() and (found == 77).all() and (mean == 77).all() and (stats == 77).all()
    for mode in outliers.MODES:
        empty = outliers.filter_cloud(torch.empty((0, 3), dtype=torch.float32, device=DEV), {"mode": mode})
        assert empty.keep.shape == (0,) and empty.counts() == (0, 0, 0, 0, 0)
    with pytest.raises(RuntimeError):
        outliers.filter_cloud(torch.zeros((4, 3)))
    with pytest.raises(RuntimeError):
        outliers.filter_cloud(pts, None, torch.ones((9,), dtype=torch.bool, device=DEV))
    with pytest.raises(RuntimeError, match="regnet_outlier_knn_f32"):
        outliers.knn_mean_distance(pts, None, 65, 0.04)


def test_a_side_stream_gives_the_same_bytes():
    from regnet_for_3d_grasping_amd import outliers
    pts = _dev(_cloud(500, 12))
    want = outliers.filter_cloud(pts, {"mode": "both", "radius": 0.02, "min_neighbours": 4, "knn": 4, "max_radius": 0.02})
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        got = outliers.filter_cloud(pts, {"mode": "both", "radius": 0.02, "min_neighbours": 4, "knn": 4, "max_radius": 0.02})
    side.synchronize()
    for name in ("keep", "status", "num", "stats", "mean_dist", "count", "found"):
        assert _bytes(getattr(got, name)) == _bytes(getattr(want, name)), name


@pytest.mark.parametrize("mode", ["radius", "both"])
def test_the_scene_equals_the_restatement(mode):
    """The CPU scene case on the device, against the restatement computed once; the last comparison is made with the device's
    own threshold."""
    from regnet_for_3d_grasping_amd import outliers
    xyz, planted, interior = ref.scene()
    want = ref.scene_result(mode)
    on_device = _dev(np.array(xyz))
    got = outliers.filter_cloud(on_device, {"mode": mode})
    again = outliers.filter_cloud(on_device, {"mode": mode})
    assert np.array_equal(got.count.cpu().numpy(), want["count"])
    if mode == "both":
        assert np.array_equal(got.found.cpu().numpy(), want["found"])
        assert np.array_equal(got.mean_dist.cpu().numpy().view(np.uint32), want["mean_dist"].view(np.uint32))
        _check_stats(got.stats.cpu().numpy(), want["mean_dist"], want["found"], 20, 2.0)
        with np.errstate(invalid="ignore"):
            assert np.array_equal(got.keep.cpu().numpy(), want["mean_dist"] <= f32(got.stats.cpu().numpy()[3]))
            decided = np.isin(want["status"], (ref.TOO_FAR, ref.KEPT))
            status = np.where(decided, np.where(got.keep.cpu().numpy(), ref.KEPT, ref.TOO_FAR), want["status"])
    else:
        status = want["status"]
    assert np.array_equal(got.status.cpu().numpy(), status)
    assert np.array_equal(got.num.cpu().numpy(), np.bincount(status, minlength=5))
    assert _bytes(got.status) == _bytes(again.status) and _bytes(got.mean_dist) == _bytes(again.mean_dist)
    assert not got.keep.cpu().numpy()[planted].any() and got.keep.cpu().numpy()[interior].all()
