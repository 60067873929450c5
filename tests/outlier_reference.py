"""numpy restatement of csrc/outlier.hip, written from the contract in include/regnet_hip.h alone.

Float32 distances in the written operation order over ALL pairs (no grid: the grid only decides which pairs the kernels look at),
counts, the k smallest by ``np.partition`` + ``sort``, ``np.sqrt`` on float32 (correctly rounded), a sequential float64 sum;
``math.fsum`` for the cloud statistics, against which the device's fixed-order sums are held within ``sum_bound``.
"""
import functools
import math

import numpy as np

QNAN_BITS = 0x7FC00000
QNAN = np.array([QNAN_BITS], dtype=np.uint32).view(np.float32)[0]
NOT_A_ROW, TOO_FEW_IN_RADIUS, TOO_FEW_NEAREST, TOO_FAR, KEPT = range(5)
BLOCK = 256


def f32(x):
    return np.float32(x)


def graph_rows(xyz, mask=None):
    """(N) bool: mask set and the three float32 coordinates finite."""
    xyz = np.asarray(xyz, dtype=np.float32)
    ok = np.isfinite(xyz).all(axis=1)
    return ok if mask is None else ok & (np.asarray(mask) != 0)


def d2_block(a, b):
    """((dx dx) + (dy dy)) + (dz dz) in float32, every operation rounded on its own: (len(a), len(b))."""
    with np.errstate(over="ignore", invalid="ignore"):
        dx = a[:, None, 0] - b[None, :, 0]
        dy = a[:, None, 1] - b[None, :, 1]
        dz = a[:, None, 2] - b[None, :, 2]
        return ((dx * dx) + (dy * dy)) + (dz * dz)


def _blocks(xyz, mask, R):
    """Yields (rows of a block of graph rows, d2 to every graph row with the row itself and everything beyond R2 at +inf)."""
    xyz = np.ascontiguousarray(np.asarray(xyz, dtype=np.float32))
    rows = np.flatnonzero(graph_rows(xyz, mask))
    pts = xyz[rows]
    R2 = f32(R) * f32(R)
    for s in range(0, len(rows), BLOCK):
        d2 = d2_block(pts[s:s + BLOCK], pts)
        within = d2 <= R2
        within[np.arange(d2.shape[0]), np.arange(s, s + d2.shape[0])] = False      # j != i, by row: a duplicate counts
        yield rows[s:s + BLOCK], np.where(within, d2, f32(np.inf))


def radius_count(xyz, mask=None, radius=0.04, min_neighbours=16):
    """count (N) int32: min(n(i), min_neighbours), -1 outside the graph."""
    count = np.full((len(xyz),), -1, dtype=np.int32)
    for rows, d2 in _blocks(xyz, mask, radius):
        count[rows] = np.minimum(np.isfinite(d2).sum(axis=1), int(min_neighbours))
    return count


def knn_mean_distance(xyz, mask=None, k=20, max_radius=0.04):
    """-> (mean_dist (N) float32, found (N) int32)."""
    k = int(k)
    n = len(xyz)
    mean = np.full((n,), QNAN, dtype=np.float32)
    found = np.full((n,), -1, dtype=np.int32)
    for rows, d2 in _blocks(xyz, mask, max_radius):
        cnt = np.isfinite(d2).sum(axis=1)
        found[rows] = np.minimum(cnt, k)
        if d2.shape[1] < k:
            continue
        smallest = np.sort(np.partition(d2, k - 1, axis=1)[:, :k], axis=1)          # ascending d2
        root = np.sqrt(smallest)                                                     # float32, correctly rounded
        S = np.zeros((d2.shape[0],), dtype=np.float64)
        for l in range(k):                                                           # one addition after the other
            S = S + root[:, l].astype(np.float64)
        m = (S / float(k)).astype(np.float32)
        full = cnt >= k
        mean[rows[full]] = m[full]
    return mean, found


def stats(mean_dist, found, k, ratio):
    """-> (n, mu, sigma, thr) over the rows with found == k: exactly rounded sums (``math.fsum``), the two-pass deviation;
    thr = float32(mu + ratio * sigma), +inf with n < 2; sigma NaN with n < 2, mu NaN with n == 0."""
    m = np.asarray(mean_dist, dtype=np.float32)[np.asarray(found) == int(k)].astype(np.float64)
    n = len(m)
    mu = math.fsum(m) / n if n else math.nan
    sigma = math.sqrt(math.fsum((m - mu) * (m - mu)) / (n - 1)) if n >= 2 else math.nan
    thr = f32(mu + float(ratio) * sigma) if n >= 2 else f32(np.inf)
    return n, mu, sigma, thr


def sum_bound(values):
    """The bound n * 2^-53 * sum|x| on the error of ANY order of float64 additions of ``values`` against their exact sum."""
    values = np.asarray(values, dtype=np.float64)
    return len(values) * 2.0 ** -53 * math.fsum(np.abs(values))


def filter_cloud(xyz, mode="radius", radius=0.04, min_neighbours=16, knn=20, max_radius=0.04, std_ratio=2.0, mask=None, thr=None):
    """-> dict(keep, status, num, count, mean_dist, found, stats).  ``thr``: the threshold to compare with instead of the
    restatement's own (the device's, whose last bits may differ within ``sum_bound``)."""
    xyz = np.asarray(xyz).astype(np.float32)
    n = len(xyz)
    out = {"count": None, "mean_dist": None, "found": None, "stats": None}
    status = None
    if mode in ("radius", "both"):
        count = radius_count(xyz, mask, radius, min_neighbours)
        keep = count == int(min_neighbours)
        status = np.where(keep, KEPT, np.where(count < 0, NOT_A_ROW, TOO_FEW_IN_RADIUS))
        mask = keep
        out["count"] = count
    if mode in ("statistical", "both"):
        mean, found = knn_mean_distance(xyz, mask, knn, max_radius)
        st = stats(mean, found, knn, std_ratio)
        with np.errstate(invalid="ignore"):
            keep = mean <= (st[3] if thr is None else f32(thr))
        second = np.where(keep, KEPT, np.where(found < 0, NOT_A_ROW, np.where(found < int(knn), TOO_FEW_NEAREST, TOO_FAR)))
        status = second if status is None else np.where(status == KEPT, second, status)
        out.update(mean_dist=mean, found=found, stats=st)
    status = status.astype(np.uint8)
    out.update(keep=keep, status=status, num=np.bincount(status, minlength=5).astype(np.int32))
    assert len(keep) == n
    return out


def apply(keep, xyz, rgb=None):
    """Copies with the removed rows at the quiet NaN (rgb: 0); dtype kept."""
    xyz = np.array(xyz, copy=True)
    xyz[~keep] = QNAN if xyz.dtype == np.float32 else np.nan
    if rgb is None:
        return xyz
    rgb = np.array(rgb, copy=True)
    rgb[~keep] = 0
    return xyz, rgb


# ---- the scene case ---------------------------------------------------------------------------------------------------------------
SCENE_W, SCENE_H = 160, 120
SCENE_K = (115.0, 115.0, 79.5, 59.5)
SCENE_PLATE_Z, SCENE_WALL_Z = 0.7, 1.0


@functools.lru_cache(maxsize=None)
def scene(seed=11, planted=12, holes=0.03, radius=0.04):
    """A rendered 160 x 120 frame -- a wall across the whole view 1 m from the camera and a plate 0.7 m from it, both facing the
    camera -- through the depth reference's deprojection, a seeded share of hole rows (NaN), and ``planted`` seeded speckle rows
    appended, each at least 2 ``radius`` from every surface point and from each other.
    -> (xyz (N,3) float32, planted (N) bool, interior (N) bool): ``interior`` marks the surface rows whose whole ``radius`` disc
    on their own surface is in view: no other surface, hole aside, and no image border within the disc's pixel radius."""
    from . import depth_reference as dr
    from . import icp_projective_reference as ipr
    rng = np.random.RandomState(seed)
    world = [ipr.rectangle((-2, -2, SCENE_WALL_Z), (4, 0, 0), (0, 4, 0)),
             ipr.rectangle((-0.2, -0.15, SCENE_PLATE_Z), (0.4, 0, 0), (0, 0.3, 0))]
    z = ipr.render(world, SCENE_W, SCENE_H, SCENE_K)[:, 2].reshape(SCENE_H, SCENE_W)
    surface = (z < 0.5 * (SCENE_PLATE_Z + SCENE_WALL_Z)).astype(np.int64)
    pts = dr.deproject(z, SCENE_K).reshape(-1, 3)
    interior = np.ones((SCENE_H, SCENE_W), dtype=bool)
    reach = np.where(surface == 1, math.ceil(radius * SCENE_K[0] / SCENE_PLATE_Z) + 1, math.ceil(radius * SCENE_K[0] / SCENE_WALL_Z) + 1)
    for dy in range(-reach.max(), reach.max() + 1):
        for dx in range(-reach.max(), reach.max() + 1):
            other = dr.shifted(surface, dy, dx, -1)
            inside = (abs(dy) <= reach) & (abs(dx) <= reach)
            interior &= ~inside | (other == surface)
    hole = rng.rand(SCENE_H * SCENE_W) < holes
    pts[hole] = QNAN
    speckle = []
    while len(speckle) < planted:          # in front of the plate: >= 0.15 m from both surfaces
        p = np.array([rng.uniform(-0.15, 0.15), rng.uniform(-0.12, 0.12), rng.uniform(0.3, 0.55)])
        if all(np.linalg.norm(p - q) >= 2.0 * radius + 1e-3 for q in speckle):
            speckle.append(p)
    xyz = np.concatenate([pts, np.asarray(speckle, dtype=np.float32)]).astype(np.float32)
    is_planted = np.arange(len(xyz)) >= len(pts)
    interior = np.concatenate([interior.reshape(-1) & ~hole, np.zeros((planted,), dtype=bool)])
    xyz.setflags(write=False)
    return xyz, is_planted, interior


@functools.lru_cache(maxsize=None)
def scene_result(mode="radius"):
    """The restatement on ``scene()`` with the defaults, computed once."""
    return filter_cloud(scene()[0], mode=mode)
