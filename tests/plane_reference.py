"""numpy restatement of the table-plane contract (DESIGN.md par. 5, include/regnet_hip.h), written from the contract text and
not from csrc/plane.hip: the counter-based draws with the retry rule, the hypotheses in individually rounded float32
operations in the written order, the gates, the inclusive sqrt-free inlier test, the winner with its tie rule, the ten float64
moments, the refit and ``table_frame``.  numpy evaluates every float32 array operation on its own (no fused multiply-add), which
is what the contract asks of the kernels.
"""
import math

import numpy as np

f32 = np.float32
MASK64 = (1 << 64) - 1
ATTEMPTS = 8


def splitmix64(x):
    """One step of splitmix64 on Python integers (exact uint64 arithmetic)."""
    x = (x + 0x9E3779B97F4A7C15) & MASK64
    z = x
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK64
    return z ^ (z >> 31)


def draw_row(seed, h, k, r, M):
    counter = (seed * (1 << 32) + (3 * h + k) * 8 + r) & MASK64
    return ((splitmix64(counter) >> 32) * M) >> 32


def to_f32(xyz):
    """The points the contract speaks of: float32 values (a float64 input rounded once) and which rows are finite."""
    with np.errstate(over="ignore"):
        p = np.ascontiguousarray(np.asarray(xyz).astype(np.float32)).reshape(-1, 3)
    return p, np.isfinite(p).all(axis=1)


def draw_triples(seed, H, M, finite):
    """(H,3) int64 row indices, -1 for an unfilled slot: the first of 8 attempts that hits a finite row."""
    idx = np.full((H, 3), -1, dtype=np.int64)
    if M == 0:
        return idx
    for h in range(H):
        for k in range(3):
            for r in range(ATTEMPTS):
                row = draw_row(seed, h, k, r, M)
                if finite[row]:
                    idx[h, k] = row
                    break
    return idx


def dot(ax, ay, az, bx, by, bz):
    """((ax bx) + (ay by)) + (az bz) in float32."""
    return (ax * bx + ay * by) + az * bz


def hypotheses(xyz, H=1024, seed=0, range=(0.0, math.inf), up_hint=None, max_tilt_deg=None):
    """-> (H,8) float32 table: n (3), p0 (3), nn, flag (0 invalid, 1 valid but gated out, 2 valid and eligible)."""
    p, finite = to_f32(xyz)
    M = len(p)
    idx = draw_triples(seed, H, M, finite)
    table = np.zeros((H, 8), dtype=np.float32)
    filled = (idx >= 0).all(axis=1)
    if not filled.any():
        return table
    rows = np.nonzero(filled)[0]
    p0, p1, p2 = p[idx[rows, 0]], p[idx[rows, 1]], p[idx[rows, 2]]
    with np.errstate(all="ignore"):
        a, b = p1 - p0, p2 - p0
        nx = a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1]
        ny = a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2]
        nz = a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]
        nn = dot(nx, ny, nz, nx, ny, nz)
        valid = (nn > f32(1e-12)) & (nn < f32(np.inf))
        g = dot(p0[:, 0], p0[:, 1], p0[:, 2], nx, ny, nz)
        gg = g * g
        lo, hi = f32(range[0]), f32(range[1])
        eligible = ((lo * lo) * nn <= gg) & (gg <= (hi * hi) * nn)
        if up_hint is not None:
            u = np.asarray(up_hint, dtype=np.float32)
            c = math.cos(math.radians(float(max_tilt_deg)))
            c2 = f32(c * c)                                   # float64, rounded once
            d = dot(nx, ny, nz, u[0], u[1], u[2])
            uu = dot(u[0], u[1], u[2], u[0], u[1], u[2])
            eligible &= d * d >= (c2 * nn) * uu
    table[rows, 0], table[rows, 1], table[rows, 2] = nx, ny, nz
    table[rows, 3:6] = p0
    table[rows, 6] = nn
    table[rows, 7] = np.where(valid, np.where(eligible, 2.0, 1.0), 0.0).astype(np.float32)
    return table


def inlier_mask(p, finite, row, threshold):
    """(M) bool: s = dot(p - p0, n), s s <= (t t) nn, inclusive; rows that are not finite take no part."""
    t = f32(threshold)
    n, q, nn = row[0:3], row[3:6], row[6]
    out = np.zeros(len(p), dtype=bool)
    pts = p[finite]
    with np.errstate(all="ignore"):
        dx, dy, dz = pts[:, 0] - q[0], pts[:, 1] - q[1], pts[:, 2] - q[2]
        s = dot(dx, dy, dz, n[0], n[1], n[2])
        out[finite] = s * s <= (t * t) * nn
    return out


def count_inliers(xyz, table, threshold=0.005):
    """(H) int32: the inlier count of every flag-2 hypothesis, -1 for the others."""
    p, finite = to_f32(xyz)
    counts = np.full(len(table), -1, dtype=np.int32)
    for h in np.nonzero(table[:, 7] == 2.0)[0]:
        counts[h] = int(inlier_mask(p, finite, table[h], threshold).sum())
    return counts


def select(counts):
    """-> (winner, count): the largest count, ties to the lower index; fewer than 3 inliers: (-1, 0)."""
    if len(counts) == 0 or counts.max() < 3:
        return -1, 0
    w = int(np.argmax(counts))                       # np.argmax returns the first maximum
    return w, int(counts[w])


def moments_of(p, mask):
    """The ten float64 sums over the inliers, coordinates widened from float32: n, Sx, Sy, Sz, Sxx, Sxy, Sxz, Syy, Syz, Szz;
    and the sums of the terms' absolute values (for the bound on the device's summation error)."""
    q = p[mask].astype(np.float64)
    x, y, z = q[:, 0], q[:, 1], q[:, 2]
    terms = [np.ones(len(q)), x, y, z, x * x, x * y, x * z, y * y, y * z, z * z]
    return np.array([t.sum() for t in terms]), np.array([np.abs(t).sum() for t in terms])


def plane_from_moments(m):
    """-> (normal, offset, rms, eigenvalues): eigh of the covariance, the smallest eigenvalue's vector, the camera origin on the
    positive side."""
    n = m[0]
    c = m[1:4] / n
    S = np.array([[m[4], m[5], m[6]], [m[5], m[7], m[8]], [m[6], m[8], m[9]]]) / n
    value, vector = np.linalg.eigh(S - np.outer(c, c))
    normal = vector[:, 0]
    offset = float(normal @ c)
    if offset > 0:
        normal, offset = -normal, -offset
    return normal, offset, math.sqrt(max(value[0], 0.0)), value


def estimate_plane(xyz, threshold=0.005, H=1024, seed=0, range=(0.0, math.inf), up_hint=None, max_tilt_deg=None):
    """The whole contract -> dict(table, counts, winner, count, mask, moments, abs_moments, normal, offset, rms, eigenvalues);
    ``winner`` -1 (and no normal) when there is no plane."""
    p, finite = to_f32(xyz)
    table = hypotheses(xyz, H, seed, range, up_hint, max_tilt_deg)
    counts = count_inliers(xyz, table, threshold)
    winner, count = select(counts)
    out = {"table": table, "counts": counts, "winner": winner, "count": count, "mask": np.zeros(len(p), dtype=bool)}
    if winner >= 0:
        out["mask"] = inlier_mask(p, finite, table[winner], threshold)
        out["moments"], out["abs_moments"] = moments_of(p, out["mask"])
        out["normal"], out["offset"], out["rms"], out["eigenvalues"] = plane_from_moments(out["moments"])
    return out


def table_frame(normal, offset, table_height=0.75):
    """z' = the plane normal; x' = the camera's x axis projected into the plane, normalised (the y axis when that projection
    is shorter than 1e-6); y' = z' x x'; translation (0, 0, table_height + the camera's distance to the plane)."""
    z = np.asarray(normal, dtype=np.float64)
    scale = np.linalg.norm(z)
    z, offset = z / scale, float(offset) / scale
    e = np.array([1.0, 0.0, 0.0])
    x = e - (e @ z) * z
    if np.linalg.norm(x) < 1e-6:
        e = np.array([0.0, 1.0, 0.0])
        x = e - (e @ z) * z
    x /= np.linalg.norm(x)
    T = np.eye(4)
    T[:3, :3] = np.stack([x, np.cross(z, x), z])
    T[2, 3] = table_height + (-offset)              # the origin's distance to the plane n . x = offset is -offset
    return T


def default_transform():
    """The default camera pose, restated: a rotation of -0.87 pi about x and the camera 1.658 m above the origin."""
    a = -0.87 * np.pi
    T = np.eye(4)
    T[:3, :3] = [[1, 0, 0], [0, np.cos(a), -np.sin(a)], [0, np.sin(a), np.cos(a)]]
    T[:3, 3] = [0.0, 0.0, 1.658]
    return T


def synthetic_frame(seed=5, width=640, height=480, noise=0.0015, holes=0.3, dtype=np.float32):
    """A seeded 640 x 480 camera frame: a table (z = 0.75 over -0.6 < x < 0.5, 0 < y < 0.9 of the table frame) with four boxes
    on it and a larger floor (z = 0) around it, seen from the default camera pose, 1.5 mm Gaussian depth noise, 30 % NaN
    holes.  -> (xyz (M,3) in camera coordinates, rgb (M,3) float64 on the 8-bit grid)."""
    rng = np.random.RandomState(seed)
    n = width * height
    x, y = rng.uniform(-0.9, 0.8, n), rng.uniform(-0.2, 1.2, n)
    z = np.where((x > -0.6) & (x < 0.5) & (y > 0) & (y < 0.9), 0.75, 0.0)
    for cx, cy, half, tall in ((-0.1, 0.4, 0.06, 0.1), (0.1, 0.5, 0.05, 0.15), (-0.2, 0.3, 0.08, 0.05), (0.0, 0.3, 0.04, 0.2)):
        z[(np.abs(x - cx) < half) & (np.abs(y - cy) < half)] = 0.75 + tall
    z = z + rng.normal(0, noise, n)
    cam = np.c_[x, y, z, np.ones(n)] @ np.linalg.inv(default_transform()).T
    xyz = cam[:, :3].astype(dtype)                   # (float64: values that float32 does not hold, rounded once by the callee)
    xyz[rng.rand(n) < holes] = np.nan
    rgb = rng.randint(0, 256, size=(n, 3)).astype(np.float64) / 255.0
    return np.ascontiguousarray(xyz), rgb
