"""Numpy restatement of the signed, capped distance field of the TSDF volume (include/regnet_hip.h "distance field": signed,
capped field; signed metres; signed query; signed margin), written from the header's text and sharing nothing with the kernel's
method -- test infrastructure, not product code.  The transform is ALL PAIRS on both sides: int64 differences of voxel indices
against the list of seed voxels (the obstacles for the positive side, the NON-obstacle voxels for the negative side), the minimum,
and of the minimisers the smallest linear index; no line pass, no separability.  The cap is a plain min / max on the uncapped
result.  The conversion to metres and the trilinear query are float32 with one operation per statement.  The classification is
``edt_reference.obstacle_mask``, the lookup ``edt_reference.lookup`` and the lattice ``approach_volume_reference``'s, imported.
"""
import numpy as np

from . import approach_volume_reference as av_ref
from . import edt_reference as edt_ref

f32 = np.float32
NONE = 1 << 30
QNAN = np.array([0x7fc00000], dtype=np.uint32).view(np.float32)[0]


def _all_pairs(seeds, dims, at=None, pairs=1 << 21):
    """``seeds`` (N) bool -> (N) int64 min over the seeds of the squared index distance (NONE without a seed), (N) int64 the
    smallest linear index that attains it (-1 without).  ``at``: linear indices -- only those voxels are computed, in that
    order (a test that reads a few voxels of a large volume)."""
    nx, ny, nz = dims
    every = edt_ref.coords(dims)
    xyz = every if at is None else every[np.asarray(at, dtype=np.int64)]
    n = len(xyz)
    idx = np.flatnonzero(seeds)                       # ascending: argmin's first hit is the smallest linear index
    dist2 = np.full((n,), NONE, dtype=np.int64)
    nearest = np.full((n,), -1, dtype=np.int64)
    if len(idx):
        q = every[idx]
        step = max(1, pairs // len(idx))
        for a in range(0, n, step):
            diff = xyz[a:a + step, None, :] - q[None, :, :]
            d = (diff * diff).sum(axis=2)
            k = d.argmin(axis=1)
            dist2[a:a + step] = d[np.arange(len(k)), k]
            nearest[a:a + step] = idx[k]
    return dist2, nearest


def transform(mask, dims, outside=False, sign=1, cap=0, at=None):
    """``mask`` (N) bool, the obstacles -> field (N) int32, nearest (N) int32.  ``at``: linear indices -- only those voxels are
    computed; the others are left 0 / -1 (0 is not a value of the field)."""
    nx, ny, nz = dims
    n = nx * ny * nz
    mask = np.asarray(mask, dtype=bool).reshape(n)
    if at is not None:
        at = np.unique(np.asarray(at, dtype=np.int64))
        field, nearest = np.zeros((n,), dtype=np.int32), np.full((n,), -1, dtype=np.int32)
        field[at], nearest[at] = _transform(mask, dims, outside, sign, cap, at)
        return field, nearest
    return _transform(mask, dims, outside, sign, cap, None)


def _transform(mask, dims, outside, sign, cap, at):
    nx, ny, nz = dims
    pos, pos_near = _all_pairs(mask, dims, at)
    mask_all = mask
    mask = mask if at is None else mask[at]
    if outside:
        xyz = edt_ref.coords(dims) if at is None else edt_ref.coords(dims)[at]
        m = np.minimum(xyz + 1, np.array([nx, ny, nz], dtype=np.int64)[None, :] - xyz).min(axis=1)
        nearer = m * m < pos                          # strictly: an interior obstacle wins a tie
        pos = np.where(nearer, m * m, pos)
        pos_near = np.where(nearer, -1, pos_near)
    field, nearest = pos, pos_near
    if sign:
        neg, neg_near = _all_pairs(~mask_all, dims, at)   # the outside is never free space
        field = np.where(mask, -neg, pos)
        nearest = np.where(mask, neg_near, pos_near)
    return apply_cap(field, nearest, cap)


def apply_cap(field, nearest, cap):
    """The cap on an uncapped result: a plain min / max, and ``nearest`` = -1 where the value is saturated STRICTLY beyond it."""
    field, nearest = np.asarray(field, dtype=np.int64), np.asarray(nearest, dtype=np.int64)
    if cap:
        c2 = int(cap) * int(cap)
        nearest = np.where(np.abs(field) > c2, -1, nearest)
        field = np.maximum(np.minimum(field, c2), -c2)
    return field.astype(np.int32), nearest.astype(np.int32)


def sdf_ref(vol_D, vol_W, dims, trunc, min_weight, margin, mode, outside, sign, cap):
    return transform(edt_ref.obstacle_mask(vol_D, vol_W, trunc, min_weight, margin, mode), dims, outside, sign, cap)


def metres_signed_ref(field, voxel):
    """a = sqrtf((float)|s|); copysignf((a - 0.5f) * voxel_f, (float)s) + 0.0f; +-inf for +-NONE."""
    s = np.asarray(field, dtype=np.int32)
    mag = np.abs(s.astype(np.int64))
    with np.errstate(all="ignore"):
        a = np.sqrt(mag.astype(np.float32))
        h = a - f32(0.5)
        m = h * f32(float(voxel))
        out = np.copysign(m, s.astype(np.float32))
        out = out + f32(0.0)
    assert out.dtype == np.float32
    return np.where(mag >= NONE, np.where(s < 0, f32(-np.inf), f32(np.inf)), out).astype(np.float32)


def _lerp(a, b, t):
    d = b - a
    s = t * d
    return a + s


def _canonical(a):
    out = np.asarray(a, dtype=np.float32).copy()
    out[np.isnan(out)] = QNAN
    return out


def world(points, T12):
    """(M,3) float32 through the 12 float32: w = (((t0 x) + (t1 y)) + (t2 z)) + t3 per row."""
    p = np.asarray(points, dtype=np.float32)
    t = np.asarray(T12, dtype=np.float32).reshape(3, 4)
    w = []
    with np.errstate(all="ignore"):
        for r in range(3):
            a = t[r, 0] * p[:, 0]
            b = t[r, 1] * p[:, 1]
            s = a + b
            b = t[r, 2] * p[:, 2]
            s = s + b
            w.append(s + t[r, 3])
    return w


def query_signed_ref(field, nearest, dims, origin, voxel, points, T12=None, interpolate=False):
    """-> distance (M) float32, gradient (M,3) float32 (NaN without ``interpolate``), nearest_xyz (M,3) float32."""
    T12 = np.eye(4, dtype=np.float32)[:3].reshape(12) if T12 is None else T12
    inside, v = edt_ref.lookup(points, T12, dims, origin, voxel)
    field = np.asarray(field, dtype=np.int32)
    nx, ny, nz = dims
    o = np.asarray(origin, dtype=np.float32)
    vx = f32(float(voxel))
    M = len(v)
    gradient = np.full((M, 3), np.nan, dtype=np.float32)
    with np.errstate(all="ignore"):
        if not interpolate:
            distance = metres_signed_ref(field[v], voxel)
        else:
            w = world(points, T12)
            lo, hi, t = [], [], []
            for k, n in enumerate((nx, ny, nz)):
                u = w[k] - o[k]
                u = u / vx
                u = u - f32(0.5)
                fl = np.floor(u)
                t.append(u - fl)
                i = np.where(inside, fl, 0).astype(np.int64)
                lo.append(np.clip(i, 0, n - 1))
                hi.append(np.clip(i + 1, 0, n - 1))
            assert all(a.dtype == np.float32 for a in t)

            def corner(z, y, x):
                return metres_signed_ref(field[(z * ny + y) * nx + x], voxel)

            c = {(a, b, d): corner((lo[2], hi[2])[a], (lo[1], hi[1])[b], (lo[0], hi[0])[d])
                 for a in (0, 1) for b in (0, 1) for d in (0, 1)}      # c[z, y, x]
            tx, ty, tz = t
            distance = _lerp(_lerp(_lerp(c[0, 0, 0], c[0, 0, 1], tx), _lerp(c[0, 1, 0], c[0, 1, 1], tx), ty),
                             _lerp(_lerp(c[1, 0, 0], c[1, 0, 1], tx), _lerp(c[1, 1, 0], c[1, 1, 1], tx), ty), tz)

            def dq(b, a):
                d = b - a
                return d / vx

            gradient[:, 0] = _lerp(_lerp(dq(c[0, 0, 1], c[0, 0, 0]), dq(c[0, 1, 1], c[0, 1, 0]), ty),
                                   _lerp(dq(c[1, 0, 1], c[1, 0, 0]), dq(c[1, 1, 1], c[1, 1, 0]), ty), tz)
            gradient[:, 1] = _lerp(_lerp(dq(c[0, 1, 0], c[0, 0, 0]), dq(c[0, 1, 1], c[0, 0, 1]), tx),
                                   _lerp(dq(c[1, 1, 0], c[1, 0, 0]), dq(c[1, 1, 1], c[1, 0, 1]), tx), tz)
            gradient[:, 2] = _lerp(_lerp(dq(c[1, 0, 0], c[0, 0, 0]), dq(c[1, 0, 1], c[0, 0, 1]), tx),
                                   _lerp(dq(c[1, 1, 0], c[0, 1, 0]), dq(c[1, 1, 1], c[0, 1, 1]), tx), ty)
            assert distance.dtype == np.float32
    distance = _canonical(np.where(inside, distance, QNAN))
    gradient = _canonical(np.where(inside[:, None], gradient, QNAN))
    xyz = np.full((M, 3), np.nan, dtype=np.float32)
    if nearest is not None:
        near = np.where(inside, np.asarray(nearest)[v], -1)
        has = near >= 0
        q = np.where(has, near, 0).astype(np.int64)
        for k, i in enumerate((q % nx, (q // nx) % ny, q // (nx * ny))):
            centre = (i.astype(np.float32) + f32(0.5)) * vx
            centre = o[k] + centre
            xyz[:, k] = np.where(has, centre, f32(np.nan))
    return distance, gradient, xyz


def margin_signed_ref(field, dims, origin, voxel, outside, L, box, standoff, step, x_extent):
    """-> margins (B,2) int32, counts (B,6) int32: every lattice sample of every grasp, nothing clipped."""
    x_lo, x_hi, ht, hw, hs, back_x = box
    x_lo, ht, hw, hs, back_x = f32(x_lo), f32(ht), f32(hw), f32(hs), f32(back_x)
    L = np.asarray(L, dtype=np.float32).reshape(-1, 12)
    B = L.shape[0]
    xh_all = np.asarray(x_hi, dtype=np.float32).reshape(-1) if np.ndim(x_hi) else np.full((B,), x_hi, dtype=np.float32)
    _, xs, _ = av_ref.lattice_counts(box, standoff, step, x_extent)
    xv, yv, zv = av_ref.lattice_samples(box, standoff, step, x_extent)
    x, y, z = np.meshgrid(xv, yv, zv, indexing="ij")
    x, y, z = x.reshape(-1), y.reshape(-1), z.reshape(-1)
    values = np.asarray(field, dtype=np.int64)
    margins = np.full((B, 2), NONE, dtype=np.int32)
    counts = np.zeros((B, 6), dtype=np.int32)
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
            inside, v = edt_ref.lookup(np.stack([x, y, z], axis=1), L[b], dims, origin, voxel)
            s = np.where(inside, values[v], -1)      # an OUTSIDE sample lies in an obstacle of unknown depth
            counted = swept & (inside | bool(outside))
            negative = counted & (s < 0)
            counts[b] = [hand.sum(), (hand & ~inside).sum(), swept.sum(), (swept & ~inside).sum(), (hand & negative).sum(),
                         negative.sum()]
            margins[b, 0] = np.min(s, initial=NONE, where=hand & counted)
            margins[b, 1] = np.min(s, initial=NONE, where=counted)
    return margins, counts
