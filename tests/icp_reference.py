"""numpy restatement of the pose-refinement contract (include/regnet_hip.h, DESIGN.md par. 5), written from the contract text and
not from csrc/icp.hip: the pose and all-pairs squared distances in float32 arithmetic step by step (every array operation on
float32 arrays, which numpy rounds one at a time), ties to the lowest target row, the 29 sums by ``math.fsum`` over float64
terms -- the exact sum, correctly rounded, which any summation order approximates -- a Cholesky solve with the contract's pivot
rule, Rodrigues, the status rules and the loop.  ``corner_scene`` is the scene the loop is tested on.
"""
import math

import numpy as np

f32 = np.float32
RUNNING, CONVERGED, MAX_ITER, TOO_FEW, DEGENERATE = range(5)
DEFAULTS = {"max_dist": 0.02, "iterations": 30, "stride": 1, "min_pairs": 100, "rot_eps": 1e-5, "trans_eps": 1e-6}
PIVOT_FLOOR = 1e-12
STATE_BYTES = 1152


def pose12(pose):
    """Rows 0..2 of a 4x4, each entry rounded once to float32."""
    with np.errstate(over="ignore"):
        return np.asarray(pose, dtype=np.float64)[:3, :].reshape(12).astype(np.float32)


def transform(xyz, pose):
    """((r0 x + r1 y) + r2 z) + r3 per coordinate, float32, every operation rounded on its own -> (n,3) float32."""
    xyz = np.asarray(xyz, dtype=np.float32).reshape(-1, 3)
    r = pose12(pose)
    x, y, z = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    with np.errstate(all="ignore"):
        p = np.stack([((r[4 * k] * x + r[4 * k + 1] * y) + r[4 * k + 2] * z) + r[4 * k + 3] for k in range(3)], axis=1)
    assert p.dtype == np.float32
    return p


def max_dist2(max_dist):
    """float32(max_dist * max_dist), the product in float64."""
    return f32(float(max_dist) * float(max_dist))


def correspond(source, target, pose, max_dist, stride=1):
    """-> (idx (rows,) int32, p (rows,3) float32): per visited source row the accepted target row, -1 rejected, -2 skipped.
    All pairs; a target row with a non-finite coordinate is never matched."""
    source = np.asarray(source, dtype=np.float32).reshape(-1, 3)[::int(stride)]
    target = np.asarray(target, dtype=np.float32).reshape(-1, 3)
    p = transform(source, pose)
    idx = np.full((len(source),), -1, dtype=np.int32)
    idx[~np.isfinite(source).all(axis=1)] = -2
    usable = np.isfinite(target).all(axis=1)
    m2 = max_dist2(max_dist)
    if not usable.any():
        return idx, p
    for k0 in range(0, len(source), 32):                 # (32 source rows at a time: the arithmetic is per element)
        rows = slice(k0, k0 + 32)
        with np.errstate(all="ignore"):
            d = p[rows, None, :] - target[None, :, :]
            d2 = ((d[:, :, 0] * d[:, :, 0]) + (d[:, :, 1] * d[:, :, 1])) + (d[:, :, 2] * d[:, :, 2])
        assert d2.dtype == np.float32
        d2 = np.where(usable[None, :], d2, f32(np.inf))
        j = np.argmin(d2, axis=1)                        # the first of equal minima: the lowest row
        best = d2[np.arange(len(j)), j]
        ok = (idx[rows] != -2) & np.isfinite(p[rows]).all(axis=1) & (best <= m2)
        idx[rows] = np.where(ok, j, idx[rows])
    return idx, p


def pair_terms(p, q, n):
    """(m,3) float32 each -> (m,28) float64: a_u a_v (u <= v, row-major), a_u r, r r with r = n . (p - q), a = (p x n, n)."""
    p, q, n = (np.asarray(v, dtype=np.float32).astype(np.float64).reshape(-1, 3) for v in (p, q, n))
    r = ((n[:, 0] * (p[:, 0] - q[:, 0])) + (n[:, 1] * (p[:, 1] - q[:, 1]))) + (n[:, 2] * (p[:, 2] - q[:, 2]))
    a = np.stack([p[:, 1] * n[:, 2] - p[:, 2] * n[:, 1], p[:, 2] * n[:, 0] - p[:, 0] * n[:, 2],
                  p[:, 0] * n[:, 1] - p[:, 1] * n[:, 0], n[:, 0], n[:, 1], n[:, 2]], axis=1)
    cols = [a[:, u] * a[:, v] for u in range(6) for v in range(u, 6)] + [a[:, u] * r for u in range(6)] + [r * r]
    return np.stack(cols, axis=1).reshape(-1, 28)


def sums(p, target, normals, idx):
    """-> (sums (29,) float64 by math.fsum, terms (pairs,28) float64)."""
    keep = idx >= 0
    j = idx[keep].astype(np.int64)
    terms = pair_terms(p[keep], np.asarray(target, dtype=np.float32).reshape(-1, 3)[j],
                       np.asarray(normals, dtype=np.float32).reshape(-1, 3)[j])
    return np.array([math.fsum(terms[:, c]) for c in range(28)] + [float(keep.sum())], dtype=np.float64), terms


def system(s):
    """The 29 sums -> (H (6,6), g (6,))."""
    H = np.zeros((6, 6))
    q = 0
    for u in range(6):
        for v in range(u, 6):
            H[u, v] = H[v, u] = s[q]
            q += 1
    return H, np.array(s[21:27], dtype=np.float64)


def cholesky_solve(H, g):
    """x with H x = -g by H = L L^T row by row, or None when a pivot L_uu^2 is not above 1e-12 * max diag(H)."""
    floor = PIVOT_FLOOR * float(np.max(np.diag(H)))
    L = np.zeros((6, 6))
    for u in range(6):
        d = H[u, u] - sum(L[u, w] * L[u, w] for w in range(u))
        if not d > floor:
            return None
        L[u, u] = math.sqrt(d)
        for r in range(u + 1, 6):
            L[r, u] = (H[r, u] - sum(L[r, w] * L[u, w] for w in range(u))) / L[u, u]
    y = np.zeros(6)
    for u in range(6):
        y[u] = (-g[u] - sum(L[u, w] * y[w] for w in range(u))) / L[u, u]
    x = np.zeros(6)
    for u in range(5, -1, -1):
        x[u] = (y[u] - sum(L[w, u] * x[w] for w in range(u + 1, 6))) / L[u, u]
    return x


def rodrigues(w):
    w = np.asarray(w, dtype=np.float64)
    th2 = (w[0] * w[0] + w[1] * w[1]) + w[2] * w[2]
    th = math.sqrt(th2)
    if th < 1e-6:
        A, B = 1.0 - th2 / 6.0, 0.5 - th2 / 24.0
    else:
        A, B = math.sin(th) / th, (1.0 - math.cos(th)) / th2
    K = np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])
    return (np.eye(3) + A * K) + B * (np.outer(w, w) - th2 * np.eye(3))


def update(pose, x):
    """[Rodrigues(x[0:3]) | x[3:6]] . pose -> (4,4) float64."""
    R = rodrigues(x[:3])
    T = np.asarray(pose, dtype=np.float64)
    out = np.eye(4)
    for u in range(3):
        for w in range(4):
            out[u, w] = (R[u, 0] * T[0, w] + R[u, 1] * T[1, w]) + R[u, 2] * T[2, w]
        out[u, 3] += x[3 + u]
    return out


def step(source, target, normals, pose, params, iteration):
    """One iteration -> (pose, status, pairs, rms, idx, sums)."""
    idx, p = correspond(source, target, pose, params["max_dist"], params["stride"])
    s, _ = sums(p, target, normals, idx)
    pairs = int(s[28])
    rms = math.sqrt(s[27] / pairs) if pairs > 0 else 0.0
    if pairs < params["min_pairs"]:
        return pose, TOO_FEW, pairs, rms, idx, s
    x = cholesky_solve(*system(s))
    if x is None:
        return pose, DEGENERATE, pairs, rms, idx, s
    pose = update(pose, x)
    status = RUNNING
    if math.sqrt(float(x[:3] @ x[:3])) < params["rot_eps"] and math.sqrt(float(x[3:] @ x[3:])) < params["trans_eps"]:
        status = CONVERGED
    elif iteration + 1 >= params["iterations"]:
        status = MAX_ITER
    return pose, status, pairs, rms, idx, s


def icp(source, target, normals, init=None, params=None):
    """The loop -> dict: ``pose`` (4,4), ``status``, ``iterations``, ``history`` (iterations,2) = (pairs, rms), ``pairs``,
    ``rms_first``, ``rms_last``."""
    p = dict(DEFAULTS)
    p.update(params or {})
    pose = np.eye(4) if init is None else np.array(init, dtype=np.float64)
    history, status, it = [], RUNNING, 0
    while status == RUNNING:
        pose, status, pairs, rms, _, _ = step(source, target, normals, pose, p, it)
        history.append((float(pairs), rms))
        it += 1
    history = np.array(history, dtype=np.float64).reshape(-1, 2)
    return {"pose": pose, "status": status, "iterations": it, "history": history, "pairs": int(history[-1, 0]),
            "rms_first": float(history[0, 1]), "rms_last": float(history[-1, 1])}


# ---- scenes -----------------------------------------------------------------------------------------------------------------
def plane_grid(axis, n=21, extent=0.2):
    """An n x n grid on the coordinate plane whose normal is ``axis`` -> (points, normals) float32."""
    u, v = np.meshgrid(np.linspace(0.0, extent, n), np.linspace(0.0, extent, n), indexing="ij")
    pts = np.zeros((n * n, 3))
    pts[:, (axis + 1) % 3], pts[:, (axis + 2) % 3] = u.reshape(-1), v.reshape(-1)
    nrm = np.zeros((n * n, 3))
    nrm[:, axis] = 1.0
    return pts.astype(np.float32), nrm.astype(np.float32)


def corner_scene(planes=3, sphere=400, seed=3):
    """Three 21 x 21 grids on the coordinate planes, 0..0.2 m, and 400 points of the octant of a 5 cm sphere about (0.1, 0.1,
    0.1), with exact normals -> (target (1723,3), normals) float32.  ``planes`` 1 or 2 and ``sphere`` 0: the degenerate scenes."""
    parts = [plane_grid(axis) for axis in (2, 0, 1)[:planes]]
    if sphere:
        rng = np.random.RandomState(seed)
        d = np.abs(rng.normal(size=(sphere, 3)))
        d /= np.linalg.norm(d, axis=1, keepdims=True)
        parts.append(((0.1 + 0.05 * d).astype(np.float32), d.astype(np.float32)))
    return np.concatenate([p for p, _ in parts]), np.concatenate([n for _, n in parts])


def perturbation(degrees=2.5, millimetres=7.0):
    """A rigid motion of that angle about (1, 2, 3) / sqrt(14) and that length along (3, -2, 1) / sqrt(14) -> (4,4) float64."""
    axis = np.array([1.0, 2.0, 3.0]) / math.sqrt(14.0)
    T = np.eye(4)
    T[:3, :3] = rodrigues(axis * math.radians(degrees))
    T[:3, 3] = np.array([3.0, -2.0, 1.0]) / math.sqrt(14.0) * (millimetres / 1000.0)
    return T


def moved_source(target, truth, every=3):
    """Every ``every``-th target point taken through the inverse of ``truth`` (float64), rounded to float32: registering it
    onto the target from the identity should return ``truth``."""
    inv = np.linalg.inv(truth)
    pts = np.asarray(target, dtype=np.float64)[::every]
    return (pts @ inv[:3, :3].T + inv[:3, 3]).astype(np.float32)


def pose_distance(a, b):
    """The largest absolute difference of the entries of two 4x4 poses."""
    return float(np.abs(np.asarray(a, dtype=np.float64) - np.asarray(b, dtype=np.float64)).max())
