"""float64 restatement of the pn2_ext / dgcnn_ext operators in numpy (test helper, not a test module).

Same surface as oracle/pn2_ext_oracle.py -- the reference's pybind entry points on CPU tensors -- for float64 data, with
the arithmetic the GPU's float64 kernels (csrc/ops_f64.hip, csrc/scatter.hip) promise:
  * distances ((dx*dx) + (dy*dy)) + (dz*dz), each operation rounded in double (numpy does not contract);
  * furthest point sampling with the reference's tie order: get_block(N) (at least 16) lanes, lane t scans t, t + block,
    ... keeping its first strict maximum (from 0 with the previous pick), then a tree that keeps the lower lane on
    equality (sampling_kernel.cu:47-117; oracle/pn2_oracle.c restates the same order in float32);
  * ball query with the radius rounded to float32, widened to double and squared in double (ball_query_kernel.cu:90);
  * 3-NN as the reference's sorted insertion from {1e40, 0, 0} / {-1, 0, 0};
  * backwards with np.add.at in ascending flattened source position (group / gather_knn: m*K + k; interpolate: n*3 + k,
    adding the rounded product g*w), from +0.0.
Vectorised over scenes and points: the loops left are the sampling picks and the 3-NN keys.
"""
import numpy as np
import torch


def _cpu64(x, name):
    if not isinstance(x, torch.Tensor) or x.is_cuda:
        raise RuntimeError("%s: the float64 reference works on CPU tensors" % name)
    if x.dtype != torch.float64:
        raise RuntimeError("%s must be float64" % name)
    return x.numpy() if x.is_contiguous() else x.contiguous().numpy()


def ref_block(n):
    """sampling_kernel.cu:32-40 (get_block) and the launch switch (:148-165): 2^ceil(log2 n), 16 <= block <= 512."""
    cnt, x = 0, n - 1
    while x > 0:
        x >>= 1
        cnt += 1
    return min(max(1 << cnt, 16), 512)


def _sqdist(ax, ay, az, bx, by, bz):
    dx, dy, dz = ax - bx, ay - by, az - bz
    s = dx * dx + dy * dy
    return s + dz * dz


def farthest_point_sample(points, num_centroids):
    p = _cpu64(points, "points")
    if p.shape[1] != 3:
        raise RuntimeError("points.size(1) does not equal to 3")
    B, _, N = p.shape
    M = int(num_centroids)
    if not M > 0:
        raise RuntimeError("num_centroids is not greater than 0")
    if not N >= M:
        raise RuntimeError("num_points is less than num_centroids")
    RB = ref_block(N)
    rows = (N + RB - 1) // RB
    ar = np.arange(B)
    temp = np.full((B, N), -1.0)
    cur = np.zeros(B, dtype=np.int64)
    out = np.zeros((B, M), dtype=np.int64)
    lane = np.arange(RB)
    dpad = np.full((B, rows * RB), -np.inf)
    for i in range(1, M):
        c = p[ar, :, cur]                                                   # (B, 3)
        d = _sqdist(p[:, 0], p[:, 1], p[:, 2], c[:, 0:1], c[:, 1:2], c[:, 2:3])
        upd = (temp > d) | (temp < 0)
        temp = np.where(upd, d, temp)
        dpad[:, :N] = temp
        cols = dpad.reshape(B, rows, RB)                                   # [b, r, t] = point r * RB + t
        best = cols.max(axis=1)                                            # (B, RB)
        first = cols.argmax(axis=1)                                        # first occurrence: the first strict maximum
        sd = np.where(best > 0, best, 0.0)
        si = np.where(best > 0, first * RB + lane[None, :], cur[:, None])
        off = RB // 2
        while off > 0:
            take = sd[:, :off] < sd[:, off:2 * off]
            sd = np.where(take, sd[:, off:2 * off], sd[:, :off])
            si = np.where(take, si[:, off:2 * off], si[:, :off])
            off //= 2
        cur = si[:, 0].astype(np.int64)
        out[:, i] = cur
    return torch.from_numpy(out)


def ball_query(points, centroids, radius, num_neighbours, chunk=256):
    p = _cpu64(points, "points")
    c = _cpu64(centroids, "centroids")
    if p.shape[1] != 3 or c.shape[1] != 3:
        raise RuntimeError("size(1) does not equal to 3")
    B, _, N1 = p.shape
    N2 = c.shape[2]
    K = int(num_neighbours)
    if K <= 0:
        raise RuntimeError("num_neighbours must be positive")
    r = np.float64(np.float32(radius))
    r2 = r * r
    index = np.zeros((B, N2, K), dtype=np.int64)
    count = np.zeros((B, N2), dtype=np.int64)
    slots = np.arange(K)
    for b in range(B):
        for m0 in range(0, N2, chunk):
            cc = c[b, :, m0:m0 + chunk]                                     # (3, n)
            d = _sqdist(p[b, 0][None, :], p[b, 1][None, :], p[b, 2][None, :], cc[0][:, None], cc[1][:, None],
                        cc[2][:, None])                                     # point minus centroid, (n, N1)
            hit = d < r2
            cs = np.cumsum(hit, axis=1)
            sel = hit & (cs <= K)
            rr, jj = np.nonzero(sel)
            idx = np.zeros((cc.shape[1], K), dtype=np.int64)
            idx[rr, cs[rr, jj] - 1] = jj
            cnt = np.minimum(cs[:, -1] if N1 else np.zeros(cc.shape[1], dtype=np.int64), K)
            firsts = np.where(cnt > 0, idx[:, 0], 0)
            index[b, m0:m0 + chunk] = np.where(slots[None, :] < cnt[:, None], idx, firsts[:, None])
            count[b, m0:m0 + chunk] = cnt
    return [torch.from_numpy(index), torch.from_numpy(count)]


def point_search(query_xyz, key_xyz, num_neighbours):
    q = _cpu64(query_xyz, "query_xyz")
    k = _cpu64(key_xyz, "key_xyz")
    B, _, N1 = q.shape
    N2 = k.shape[2]
    if k.shape[0] != B or q.shape[1] != 3 or k.shape[1] != 3:
        raise RuntimeError("point_search: shape mismatch")
    if num_neighbours != 3:
        raise RuntimeError("num_neighbours does not equal to K")
    if N2 < 3:
        raise RuntimeError("num_key is less than num_neighbours")
    md = [np.full((B, N1), 1e40), np.zeros((B, N1)), np.zeros((B, N1))]
    mi = [np.full((B, N1), -1, dtype=np.int64), np.zeros((B, N1), dtype=np.int64), np.zeros((B, N1), dtype=np.int64)]
    for j in range(N2):
        d = _sqdist(q[:, 0], q[:, 1], q[:, 2], k[:, 0, j:j + 1], k[:, 1, j:j + 1], k[:, 2, j:j + 1])   # query minus key
        s0 = d < md[0]
        s1 = ~s0 & (d < md[1])
        s2 = ~s0 & ~s1 & (d < md[2])
        md[2] = np.where(s0 | s1, md[1], np.where(s2, d, md[2]))
        mi[2] = np.where(s0 | s1, mi[1], np.where(s2, j, mi[2]))
        md[1] = np.where(s0, md[0], np.where(s1, d, md[1]))
        mi[1] = np.where(s0, mi[0], np.where(s1, j, mi[1]))
        md[0] = np.where(s0, d, md[0])
        mi[0] = np.where(s0, j, mi[0])
    return [torch.from_numpy(np.stack(mi, axis=2)), torch.from_numpy(np.stack(md, axis=2))]


def _gather(x, idx):
    """x (C, N), idx (...) -> (C, ...): x[:, idx], an index outside [0, N) reads as 0."""
    ok = (idx >= 0) & (idx < x.shape[1])
    return np.where(ok[None], x[:, np.where(ok, idx, 0)], 0.0)


def _scatter(vals, idx, R):
    """vals (C, L), idx (L,) -> (C, R): np.add.at in ascending source position from +0.0; indices outside [0, R) skipped."""
    ok = (idx >= 0) & (idx < R)
    acc = np.zeros((R, vals.shape[0]))
    np.add.at(acc, idx[ok], vals[:, ok].T)
    return acc.T


def group_points_forward(input, index):
    x = _cpu64(input, "input")
    idx = index.contiguous().numpy()
    if x.ndim != 3 or idx.ndim != 3 or idx.shape[0] != x.shape[0]:
        raise RuntimeError("group_points_forward: shape mismatch")
    return torch.from_numpy(np.stack([_gather(x[b], idx[b]) for b in range(x.shape[0])]) if x.shape[0] else
                            np.zeros((0, x.shape[1]) + idx.shape[1:]))


def group_points_backward(grad_output, index, num_points):
    g = _cpu64(grad_output, "grad_output")
    idx = index.contiguous().numpy()
    B, C, N2, K = g.shape
    if idx.shape != (B, N2, K):
        raise RuntimeError("group_points_backward: shape mismatch")
    out = np.zeros((B, C, int(num_points)))
    for b in range(B):
        out[b] = _scatter(g[b].reshape(C, N2 * K), idx[b].reshape(-1), int(num_points))
    return torch.from_numpy(out)


def interpolate_forward(input, index, weight):
    x = _cpu64(input, "input")
    w = _cpu64(weight, "weight")
    idx = index.contiguous().numpy()
    B, C, M = x.shape
    N = idx.shape[1]
    if idx.shape[0] != B or idx.shape[2] != 3 or w.shape != (B, N, 3):
        raise RuntimeError("interpolate_forward: shape mismatch")
    out = np.zeros((B, C, N))
    for b in range(B):
        acc = np.zeros((C, N))
        for k in range(3):
            acc = acc + _gather(x[b], idx[b, :, k]) * w[b, :, k][None, :]
        out[b] = acc
    return torch.from_numpy(out)


def interpolate_backward(grad_output, index, weight, num_inst):
    g = _cpu64(grad_output, "grad_output")
    w = _cpu64(weight, "weight")
    idx = index.contiguous().numpy()
    B, C, N = g.shape
    if idx.shape != (B, N, 3) or w.shape != (B, N, 3):
        raise RuntimeError("interpolate_backward: shape mismatch")
    out = np.zeros((B, C, int(num_inst)))
    for b in range(B):
        vals = (g[b][:, :, None] * w[b][None, :, :]).reshape(C, N * 3)     # position n*3 + k, rounded products
        out[b] = _scatter(vals, idx[b].reshape(-1), int(num_inst))
    return torch.from_numpy(out)


# dgcnn_ext surface (functions/csrc/main.cpp:3-6): the same gather / scatter-add.
def gather_knn_forward(input, index):
    return group_points_forward(input, index)


def gather_knn_backward(grad_output, index):
    return group_points_backward(grad_output, index, grad_output.size(2))
