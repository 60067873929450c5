"""Numpy restatement of the distance field of the TSDF volume (include/regnet_hip.h "distance field"; csrc/edt.hip), written from
the header's text and sharing nothing with the kernel's method -- test infrastructure, not product code.  The transform is ALL
PAIRS: int64 differences of voxel indices against the list of obstacle voxels, the minimum, and of the minimisers the smallest
linear index; no line pass, no separability.  The classification is the approach analysis' (restated here on whole planes), the
lattice and the lookup of the query and the margin are ``approach_volume_reference``'s, imported.
"""
import numpy as np

from . import approach_volume_reference as av_ref

f32 = np.float32
NONE = 1 << 30
MODES = ("solid", "solid_or_unseen")


def obstacle_mask(vol_D, vol_W, trunc, min_weight, margin, mode):
    """-> (N) bool: UNKNOWN = W < min_weight or D NaN; SOLID = known and D < float32(margin / trunc); mode 0: SOLID, 1: either."""
    D = np.asarray(vol_D, dtype=np.float32)
    W = np.asarray(vol_W)
    d_solid = f32(float(margin) / float(trunc))
    with np.errstate(invalid="ignore"):
        unknown = (W < np.int32(min_weight)) | np.isnan(D)
        solid = ~unknown & (D < d_solid)
    return solid | unknown if int(mode) == 1 else solid


def coords(dims):
    """-> (N,3) int64: (ix, iy, iz) of every linear index l = (iz ny + iy) nx + ix."""
    nx, ny, nz = dims
    l = np.arange(nx * ny * nz, dtype=np.int64)
    return np.stack([l % nx, (l // nx) % ny, l // (nx * ny)], axis=1)


def transform(mask, dims, outside=False, at=None, pairs=1 << 21):
    """``mask`` (N) bool -> dist2 (N) int32, nearest (N) int32, by all pairs.  ``at``: linear indices -- only those voxels are
    computed (the others are left NONE / -1): for a test that reads a few voxels of a large volume."""
    nx, ny, nz = dims
    n = nx * ny * nz
    mask = np.asarray(mask, dtype=bool).reshape(n)
    if at is not None:
        at = np.unique(np.asarray(at, dtype=np.int64))
        d2, near = transform(mask, dims, outside, None, pairs) if len(at) == n else _transform_rows(mask, dims, outside, at, pairs)
        dist2, nearest = np.full((n,), NONE, dtype=np.int32), np.full((n,), -1, dtype=np.int32)
        dist2[at], nearest[at] = (d2[at], near[at]) if len(at) == n else (d2, near)
        return dist2, nearest
    return _transform_rows(mask, dims, outside, np.arange(n, dtype=np.int64), pairs)


def _transform_rows(mask, dims, outside, rows, pairs):
    nx, ny, nz = dims
    n = len(rows)
    xyz = coords(dims)[rows]
    obstacles = np.flatnonzero(mask)                 # ascending linear index: argmin's first hit is the smallest
    dist2 = np.full((n,), NONE, dtype=np.int64)
    nearest = np.full((n,), -1, dtype=np.int64)
    if len(obstacles):
        q = coords(dims)[obstacles]
        step = max(1, pairs // len(obstacles))     # voxels per block: the block's pair table stays small
        for a in range(0, n, step):
            diff = xyz[a:a + step, None, :] - q[None, :, :]
            d = (diff * diff).sum(axis=2)
            k = d.argmin(axis=1)
            dist2[a:a + step] = d[np.arange(len(k)), k]
            nearest[a:a + step] = obstacles[k]
    if outside:
        m = np.minimum(xyz + 1, np.array([nx, ny, nz], dtype=np.int64)[None, :] - xyz).min(axis=1)
        nearer = m * m < dist2                       # strictly: an interior obstacle wins a tie
        dist2 = np.where(nearer, m * m, dist2)
        nearest = np.where(nearer, -1, nearest)
    return dist2.astype(np.int32), nearest.astype(np.int32)


def edt_ref(vol_D, vol_W, dims, trunc, min_weight, margin, mode, outside):
    return transform(obstacle_mask(vol_D, vol_W, trunc, min_weight, margin, mode), dims, outside)


def metres_ref(dist2, voxel):
    """sqrtf((float)d2) * voxel_f, + 0.0f; +inf for NONE."""
    d2 = np.asarray(dist2, dtype=np.int32)
    with np.errstate(all="ignore"):
        root = np.sqrt(d2.astype(np.float32))
        out = root * f32(float(voxel))
        out = out + f32(0.0)
    return np.where(d2 >= NONE, f32(np.inf), out).astype(np.float32)


def lookup(points, T12, dims, origin, voxel):
    """``points`` (M,3) float32 through the 12 float32 ``T12`` -> inside (M) bool, v (M) int64 (0 where not inside)."""
    p = np.asarray(points, dtype=np.float32)
    t = np.asarray(T12, dtype=np.float32).reshape(3, 4)
    o = np.asarray(origin, dtype=np.float32)
    vx = f32(float(voxel))
    c = []
    with np.errstate(all="ignore"):
        for r in range(3):
            a = t[r, 0] * p[:, 0]
            b = t[r, 1] * p[:, 1]
            s = a + b
            b = t[r, 2] * p[:, 2]
            s = s + b
            w = s + t[r, 3]
            w = w - o[r]
            w = w / vx
            c.append(np.floor(w))
        assert all(a.dtype == np.float32 for a in c)
        nx, ny, nz = dims
        inside = ((c[0] >= 0) & (c[0] < f32(nx)) & (c[1] >= 0) & (c[1] < f32(ny)) & (c[2] >= 0) & (c[2] < f32(nz)))
        ix, iy, iz = (np.where(inside, a, 0).astype(np.int64) for a in c)
    return inside, (iz * ny + iy) * nx + ix


def query_ref(dist2, nearest, dims, origin, voxel, points, T12=None):
    """-> distance (M) float32, nearest_xyz (M,3) float32 (all NaN when ``nearest`` is None)."""
    T12 = np.eye(4, dtype=np.float32)[:3].reshape(12) if T12 is None else T12
    inside, v = lookup(points, T12, dims, origin, voxel)
    nx, ny, _ = dims
    distance = np.where(inside, metres_ref(np.asarray(dist2)[v], voxel), f32(np.nan)).astype(np.float32)
    xyz = np.full((len(v), 3), np.nan, dtype=np.float32)
    if nearest is not None:
        near = np.where(inside, np.asarray(nearest)[v], -1)
        has = near >= 0
        q = np.where(has, near, 0).astype(np.int64)
        o = np.asarray(origin, dtype=np.float32)
        vx = f32(float(voxel))
        for k, i in enumerate((q % nx, (q // nx) % ny, q // (nx * ny))):
            centre = (i.astype(np.float32) + f32(0.5)) * vx
            centre = o[k] + centre
            xyz[:, k] = np.where(has, centre, f32(np.nan))
    return distance, xyz


def margin_ref(dist2, dims, origin, voxel, outside, L, box, standoff, step, x_extent):
    """-> margins (B,2) int32, counts (B,4) int32: every lattice sample of every grasp, nothing clipped."""
    x_lo, x_hi, ht, hw, hs, back_x = box
    x_lo, ht, hw, hs, back_x = f32(x_lo), f32(ht), f32(hw), f32(hs), f32(back_x)
    L = np.asarray(L, dtype=np.float32).reshape(-1, 12)
    B = L.shape[0]
    xh_all = np.asarray(x_hi, dtype=np.float32).reshape(-1) if np.ndim(x_hi) else np.full((B,), x_hi, dtype=np.float32)
    (n_x, n_y, n_z), xs, _ = av_ref.lattice_counts(box, standoff, step, x_extent)
    xv, yv, zv = av_ref.lattice_samples(box, standoff, step, x_extent)
    x, y, z = np.meshgrid(xv, yv, zv, indexing="ij")
    x, y, z = x.reshape(-1), y.reshape(-1), z.reshape(-1)
    d2_all = np.asarray(dist2, dtype=np.int64)
    margins = np.full((B, 2), NONE, dtype=np.int32)
    counts = np.zeros((B, 4), dtype=np.int32)
    with np.errstate(all="ignore"):
        section = (z < ht) & (z > -ht) & (y < hw) & (y > -hw)
        inner = section & (y < hs) & (y > -hs)
        for b in range(B):
            xh = xh_all[b]
            close = (x > x_lo) & (x < xh)
            back = section & close & (x < back_x)
            finger = section & close & ((y > hs) | (y < -hs))
            front = np.where(inner, back_x, xh).astype(np.float32)
            blocker = section & (x < front) & (x > xs)
            hand = back | finger
            swept = hand | blocker
            inside, v = lookup(np.stack([x, y, z], axis=1), L[b], dims, origin, voxel)
            d2 = np.where(inside, d2_all[v], 0)
            counted = swept & (inside | bool(outside))
            counts[b] = [hand.sum(), (hand & ~inside).sum(), swept.sum(), (swept & ~inside).sum()]
            margins[b, 0] = np.min(d2, initial=NONE, where=hand & counted)
            margins[b, 1] = np.min(d2, initial=NONE, where=counted)
    return margins, counts
