"""The contract of the region-grouping kernels (csrc/region.hip) restated in numpy, from the kernel comments and
``region_ops``' docstrings: float32 where the kernel is float32 (numpy rounds every float32 operation on its own, there is no
contraction), float64 where a sum is checked.  Index lists are compared exactly, so every membership test is written in the
kernel's order of operations.

  radius      d2 = ((dx dx) + (dy dy)) + (dz dz), d = point - centre (``sqdist3`` of csrc/common.h: three individually rounded
              products summed left to right); member iff d2 <= T (inclusive); members in ascending index order
  box         t = R (p - c) with rows summed as (m0 dx + m1 dy) + m2 dz; member iff 0 < t.x < xlim, |t.y| < ylim,
              |t.z| < zlim -- all six faces strict
  resample    index = cand[pos], points = pc[index]; pos < 0: -1 / -1.0; pos >= cap or a candidate outside [0, N): -1 / -1.0
              and the out-of-range flag
  gather_max  max over the group's rows; ids outside [0, num_rows) are skipped; nothing left: -inf.  Scene form: a local id
              >= 0 is moved by (row id // per_scene) * scene_stride first
  gather_max_arg   a negative id counts from the end; what is still outside is skipped; the FIRST position in group order that
              attains the maximum gives ``arg`` (the row id); nothing left: -inf / -1
  scatter_max_grad grad[b * batch_stride + n * row_stride + f * ch_stride] += dy[r, f], b = arg // scene_rows,
              n = arg % scene_rows, arg < 0 skipped; float64
  rowsum_neg  -(sum of K contiguous floats); float64

The second half builds the inputs of tests/test_gpu_region_edges.py; tests/test_region_reference_cpu.py asserts on the CPU that
every builder really contains what it is for (a point on each boundary, an empty wave quarter, ...).
"""
import numpy as np

f32 = np.float32
INF32 = f32(np.inf)
RG_WAVES = 4            # waves per centre of radius_group_kernel / grasps per workgroup of box_crop_kernel


def sqdist3(p, c):
    """p (..., >= 3), c (>= 3,) float32 -> ((dx dx) + (dy dy)) + (dz dz) with d = p - c, every operation rounded to float32."""
    p, c = np.asarray(p, dtype=f32), np.asarray(c, dtype=f32)
    dx, dy, dz = p[..., 0] - c[0], p[..., 1] - c[1], p[..., 2] - c[2]
    xx, yy, zz = dx * dx, dy * dy, dz * dz
    s = xx + yy
    return s + zz


def _lists(members, width):
    """list of ascending index arrays -> zero-padded (len, width) int32 lists and their lengths."""
    cand = np.zeros((len(members), max(width, 1)), dtype=np.int32)
    count = np.zeros((len(members),), dtype=np.int32)
    for i, m in enumerate(members):
        count[i] = len(m)
        cand[i, :len(m)] = m
    return cand, count


def radius_candidates(pc, centres, T):
    """pc (B,N,C>=3), centres (B,Nc,C'>=3) float32, T the float32 threshold on d2 -> cand (B,Nc,max(N,1)) int32 (the first
    ``count`` entries are the members, ascending; 0 behind them), count (B,Nc) int32."""
    pc, centres = np.asarray(pc, dtype=f32), np.asarray(centres, dtype=f32)
    B, N = pc.shape[:2]
    Nc = centres.shape[1]
    T = f32(T)
    members = [np.nonzero(sqdist3(pc[b, :, :3], centres[b, c, :3]) <= T)[0] for b in range(B) for c in range(Nc)]
    cand, count = _lists(members, N)
    return cand.reshape(B, Nc, -1), count.reshape(B, Nc)


def box_candidates(group_points, centre, rot, xlim, ylim, zlim):
    """group_points (n,G,C>=3), centre (n,3), rot (n,3,3) rows [approach; axis_y; minor_normal], xlim / ylim (n), zlim ->
    cand (n,max(G,1)) int32 ascending in-box positions, count (n) int32."""
    p = np.asarray(group_points, dtype=f32)[:, :, :3]
    c, m = np.asarray(centre, dtype=f32), np.asarray(rot, dtype=f32).reshape(-1, 3, 3)
    xl, yl, zl = np.asarray(xlim, dtype=f32), np.asarray(ylim, dtype=f32), f32(zlim)
    n, G = p.shape[:2]
    members = []
    for i in range(n):
        dx, dy, dz = p[i, :, 0] - c[i, 0], p[i, :, 1] - c[i, 1], p[i, :, 2] - c[i, 2]
        tx = (m[i, 0, 0] * dx + m[i, 0, 1] * dy) + m[i, 0, 2] * dz
        ty = (m[i, 1, 0] * dx + m[i, 1, 1] * dy) + m[i, 1, 2] * dz
        tz = (m[i, 2, 0] * dx + m[i, 2, 1] * dy) + m[i, 2, 2] * dz
        inside = (tx > 0) & (tx < xl[i]) & (ty > -yl[i]) & (ty < yl[i]) & (tz > -zl) & (tz < zl)
        members.append(np.nonzero(inside)[0])
    return _lists(members, G)


def resample_groups(pc, cand, pos):
    """pc (B,N,C) float32, cand (B,Nc,cap) int32, pos (B,Nc,G) int64 -> index (B,Nc,G) int64, points (B,Nc,G,C) float32 and
    whether the out-of-range flag is raised."""
    pc, cand, pos = np.asarray(pc, dtype=f32), np.asarray(cand), np.asarray(pos)
    N, C = pc.shape[1:]
    cap = cand.shape[2]
    index = np.full(pos.shape, -1, dtype=np.int64)
    points = np.full(pos.shape + (C,), -1.0, dtype=f32)
    flag = False
    for b, c, g in np.ndindex(*pos.shape):
        p = int(pos[b, c, g])
        if p < 0:
            continue
        j = int(cand[b, c, p]) if p < cap else -1
        if j < 0 or j >= N:
            flag = True
            continue
        index[b, c, g] = j
        points[b, c, g] = pc[b, j]
    return index, points, flag


def gather_max(feat, rows, num_rows=None, row_ids=None, per_scene=0, scene_stride=0):
    """feat (>= num_rows, F) float32, rows (R_all,G) int64 -> (R,F) float32.  ``row_ids`` (R,) selects the lists (None: all, in
    order); per_scene > 0: the ids of list ``rid`` are local to scene rid // per_scene, whose rows start at scene * scene_stride."""
    feat, rows = np.asarray(feat, dtype=f32), np.asarray(rows)
    num_rows = feat.shape[0] if num_rows is None else num_rows
    rids = np.arange(rows.shape[0]) if row_ids is None else np.asarray(row_ids)
    out = np.full((len(rids), feat.shape[1]), -np.inf, dtype=f32)
    for r, rid in enumerate(rids):
        base = (int(rid) // per_scene) * scene_stride if per_scene > 0 else 0
        for j in rows[rid]:
            j = int(j)
            if j < 0:
                continue
            j += base
            if j < num_rows:
                out[r] = np.maximum(out[r], feat[j])
    return out


def gather_max_arg(feat, rows, last_wins=False):
    """feat (num_rows,F) float32, rows (R,G) int64 -> out (R,F) float32, arg (R,F) int64: the row that gave the maximum, the
    first position in group order among equals.  ``last_wins`` is the WRONG rule (the last position among equals); the CPU
    tests use it to show that their inputs tell the two apart."""
    feat, rows = np.asarray(feat, dtype=f32), np.asarray(rows)
    num_rows, F = feat.shape
    R = rows.shape[0]
    out = np.full((R, F), -np.inf, dtype=f32)
    arg = np.full((R, F), -1, dtype=np.int64)
    for r in range(R):
        for j in rows[r]:
            j = int(j)
            if j < 0:
                j += num_rows
            if j < 0 or j >= num_rows:
                continue
            v = feat[j]
            take = (arg[r] < 0) | ((v >= out[r]) if last_wins else (v > out[r]))
            out[r] = np.where(take, v, out[r])
            arg[r] = np.where(take, j, arg[r])
    return out, arg


def scatter_max_grad(dy, arg, grad_shape, scene_rows, batch_stride, row_stride, ch_stride):
    """dy (R,F), arg (R,F) int64 -> float64 array of ``grad_shape`` (a zero gradient plus every dy[r,f] at its address)."""
    dy, arg = np.asarray(dy, dtype=np.float64), np.asarray(arg, dtype=np.int64)
    flat = np.zeros(int(np.prod(grad_shape)), dtype=np.float64)
    f = np.broadcast_to(np.arange(arg.shape[1], dtype=np.int64), arg.shape)
    keep = arg >= 0
    b, n = arg[keep] // scene_rows, arg[keep] % scene_rows
    np.add.at(flat, b * batch_stride + n * row_stride + f[keep] * ch_stride, dy[keep])
    return flat.reshape(grad_shape)


def rowsum_neg(x):
    """x (..., K) -> -(sum over the last axis) in float64."""
    return -np.asarray(x, dtype=np.float64).sum(axis=-1)


# ---- test inputs ----------------------------------------------------------------------------------------------------------
RADIUS_N = (1, 3, 63, 64, 65, 255, 256, 257, 1023, 1025, 4099)
RADIUS_LAYOUTS = ("uniform", "quarter0", "quarter1", "quarter2", "quarter3", "last", "all", "none")
FAR = 100.0


def quarter_bounds(N):
    """[beg, end) of the cloud quarters the four waves of a centre walk: ceil(ceil(N / 4) / 64) * 64 points each, cut at N."""
    per = ((N + RG_WAVES - 1) // RG_WAVES + 63) // 64 * 64
    return [(min(N, w * per), min(N, min(N, w * per) + per)) for w in range(RG_WAVES)]


def radius_case(layout, B, N, Nc, seed):
    """-> pc (B,N,6), centres (B,Nc,6) float32 and the float32-rounded radius.
    uniform: members wherever they fall; quarterQ: only points of wave quarter Q are near a centre (point j near centre
    j % Nc), every other point ~FAR away; last: only point N - 1; all: a radius that takes every point; none: centres away
    from every point."""
    rng = np.random.default_rng(seed)
    pc = rng.uniform(-0.4, 0.4, (B, N, 6)).astype(f32)
    centres = rng.uniform(-0.3, 0.3, (B, Nc, 6)).astype(f32)
    radius = 0.25
    if layout == "all":
        radius = 1000.0
    elif layout == "none":
        radius = 1e-4
        centres[:, :, :3] += f32(5.0)
    elif layout != "uniform":
        radius = 0.05
        pc[:, :, :3] += f32(FAR)
        beg, end = (N - 1, N) if layout == "last" else quarter_bounds(N)[int(layout[-1])]
        for b in range(B):
            for j in range(beg, end):
                pc[b, j, :3] = centres[b, j % Nc, :3] + rng.uniform(-0.02, 0.02, 3).astype(f32)
    return pc, centres, float(f32(radius))


# the radii the pipeline groups with (get_regiondataset.group_radius(0.08, 0.01, 0.06, r_time) = float32(0.08 * r_time), r_time
# 0.1 and 0.8), the gripper's 0.06 and 0.08 themselves and three round numbers
BOUNDARY_RADII = (0.06, 0.08, float(f32(0.08 * 0.1)), float(f32(0.08 * 0.8)), 0.03125, 0.25, 1.0)


def radius_boundary_case(radius, seed=0, shell=4000):
    """One centre at the origin.  Points 0..17: (+-v, 0, 0), (0, +-v, 0), (0, 0, +-v) for v = r, the next float32 above, the
    next below.  Behind them ``shell`` points in random directions at r (1 + k 2^-24), k = -4..4: their d2 fall on the few
    float32 values around the threshold, the threshold itself and its two neighbours among them (asserted on the CPU).
    -> pc (1,18 + shell,6), centres (1,1,6), float(r)."""
    r = f32(radius)
    rng = np.random.default_rng(seed)
    pts = []
    for axis in range(3):
        for sign in (1.0, -1.0):
            for v in (r, np.nextafter(r, INF32), np.nextafter(r, -INF32)):
                p = np.zeros(3, dtype=f32)
                p[axis] = f32(sign) * v
                pts.append(p)
    d = rng.standard_normal((shell, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    k = rng.integers(-4, 5, shell)
    pts = np.concatenate([np.stack(pts), (d * (np.float64(r) * (1.0 + k * 2.0 ** -24))[:, None]).astype(f32)])
    pc = np.zeros((1, len(pts), 6), dtype=f32)
    pc[0, :, :3] = pts
    pc[0, :, 3:] = rng.uniform(-1, 1, (len(pts), 3)).astype(f32)
    return pc, np.zeros((1, 1, 6), dtype=f32), float(r)


CAPACITY_COUNTS = (0, 1, 63, 64, 65, 99, 100, 101, 300)
CAPACITIES = (0, 1, 64, 100)


def capacity_case(seed, B=2, N=1027):
    """Centre c of every scene has exactly CAPACITY_COUNTS[c] members, scattered over the whole cloud (every wave quarter):
    counts below, at and above every capacity of CAPACITIES.  -> pc (B,N,6), centres (B,Nc,6), radius."""
    rng = np.random.default_rng(seed)
    Nc = len(CAPACITY_COUNTS)
    pc = rng.uniform(-0.4, 0.4, (B, N, 6)).astype(f32)
    pc[:, :, 1] += f32(500.0)
    centres = np.zeros((B, Nc, 6), dtype=f32)
    centres[:, :, 0] = 10.0 * np.arange(Nc, dtype=f32)
    for b in range(B):
        order, used = rng.permutation(N), 0
        for c, k in enumerate(CAPACITY_COUNTS):
            ids = order[used:used + k]
            used += k
            pc[b, ids, :3] = centres[b, c, :3] + rng.uniform(-0.02, 0.02, (k, 3)).astype(f32)
    return pc, centres, float(f32(0.05))


BOX_N = (1, 3, 4, 5, 9)
BOX_G = (1, 63, 64, 65, 200, 1024)


def box_case(kind, n, G, seed):
    """kind random / inside / outside -> group_points (n,G,6), centre (n,3), rot (n,3,3), xlim (n), ylim (n) float32, zlim.
    The points are drawn in the gripper frame and turned into the scene frame (p = R^T t + c in float64, then rounded);
    inside / outside keep 10 % of a limit away from every face, so rounding cannot move a point across one."""
    rng = np.random.default_rng(seed)
    q, _ = np.linalg.qr(rng.standard_normal((n, 3, 3)))
    centre = rng.uniform(-0.01, 0.01, (n, 3))
    xl, yl, zl = rng.uniform(0.02, 0.04, n), rng.uniform(0.02, 0.04, n), 0.01
    if kind == "random":
        t = rng.uniform(-0.05, 0.05, (n, G, 3))
        t[:, :, 2] *= 0.4
    else:
        t = np.stack([rng.uniform(0.1, 0.9, (n, G)) * xl[:, None], rng.uniform(-0.9, 0.9, (n, G)) * yl[:, None],
                      rng.uniform(-0.9, 0.9, (n, G)) * zl], axis=2)
        if kind == "outside":           # one coordinate of every point goes beyond its face
            which = rng.integers(0, 4, (n, G))
            t[:, :, 0] = np.where(which == 0, -t[:, :, 0], np.where(which == 1, 1.1 * xl[:, None] + t[:, :, 0], t[:, :, 0]))
            t[:, :, 1] = np.where(which == 2, np.sign(t[:, :, 1] + 1e-30) * 1.1 * yl[:, None] + t[:, :, 1], t[:, :, 1])
            t[:, :, 2] = np.where(which == 3, np.sign(t[:, :, 2] + 1e-30) * 1.1 * zl + t[:, :, 2], t[:, :, 2])
    pts = np.zeros((n, G, 6), dtype=f32)
    pts[:, :, :3] = (np.einsum("nji,ngj->ngi", q, t) + centre[:, None, :]).astype(f32)
    pts[:, :, 3:] = rng.uniform(-1, 1, (n, G, 3)).astype(f32)
    return pts, centre.astype(f32), q.astype(f32), xl.astype(f32), yl.astype(f32), float(f32(zl))


def box_strict_case(seed=0, G=70):
    """Identity rotation and a zero centre, so t == p exactly.  Every grasp gets 20 special points at random positions of its
    G: on each of the six faces (out), the inward float32 neighbour of each (in), the outward neighbour (out), and around
    t.x = 0: +0, -0 (out), the smallest subnormal and the smallest normal float32 (in), the negative subnormal (out).  The other
    positions hold a point in the middle of the box or one behind the gripper.
    -> group_points (n,G,6), centre, rot, xlim, ylim, zlim, inside (n,G) bool: the expected membership, by construction."""
    rng = np.random.default_rng(seed)
    xlim = np.array([0.03, 0.02, 0.04, 0.025, 0.035], dtype=f32)
    ylim = np.array([0.02, 0.04, 0.03, 0.035, 0.025], dtype=f32)
    zl = f32(0.005)
    n = len(xlim)
    tiny, sub = np.finfo(f32).tiny, np.nextafter(f32(0), f32(1))
    zero = f32(0)
    pts = np.zeros((n, G, 6), dtype=f32)
    inside = np.zeros((n, G), dtype=bool)
    for i in range(n):
        xl, yl = xlim[i], ylim[i]
        mid = xl / f32(2)
        special = [((zero, zero, zero), False), ((-zero, zero, zero), False), ((sub, zero, zero), True), ((tiny, zero, zero), True),
                   ((-sub, zero, zero), False), ((xl, zero, zero), False), ((np.nextafter(xl, zero), zero, zero), True),
                   ((np.nextafter(xl, INF32), zero, zero), False)]
        for sign in (f32(1), f32(-1)):
            special += [((mid, sign * yl, zero), False), ((mid, sign * np.nextafter(yl, zero), zero), True),
                        ((mid, sign * np.nextafter(yl, INF32), zero), False),
                        ((mid, zero, sign * zl), False), ((mid, zero, sign * np.nextafter(zl, zero)), True),
                        ((mid, zero, sign * np.nextafter(zl, INF32)), False)]
        fill = rng.integers(0, 2, G).astype(bool)
        pts[i, :, 0] = np.where(fill, mid, -xl)
        inside[i] = fill
        for slot, (p, member) in zip(rng.permutation(G)[:len(special)], special):
            pts[i, slot, :3] = p
            inside[i, slot] = member
    pts[:, :, 3:] = rng.uniform(-1, 1, (n, G, 3)).astype(f32)
    rot = np.broadcast_to(np.eye(3, dtype=f32), (n, 3, 3)).copy()
    return pts, np.zeros((n, 3), dtype=f32), rot, xlim, ylim, float(zl), inside


RESAMPLE_SHAPES = ((2, 3, 7), (1, 1, 1), (2, 5, 37), (3, 4, 65))     # (B, Nc, G): B Nc G = 42, 1, 370, 780, none a multiple of 256
RESAMPLE_C = (3, 6, 64)


def resample_case(B, Nc, G, C, seed, N=53, cap=40):
    """-> pc (B,N,C) float32, cand (B,Nc,cap) int32, pos (B,Nc,G) int64, all in range: candidate lists of random lengths
    (garbage behind them), centre (B-1, Nc-1) without candidates (pos -1), positions up to the last list entry."""
    rng = np.random.default_rng(seed)
    pc = rng.uniform(-1, 1, (B, N, C)).astype(f32)
    cand = np.full((B, Nc, cap), 2 ** 30, dtype=np.int32)
    pos = np.empty((B, Nc, G), dtype=np.int64)
    for b in range(B):
        for c in range(Nc):
            k = int(rng.integers(1, cap + 1))
            cand[b, c, :k] = np.sort(rng.choice(N, k, replace=False))
            pos[b, c] = rng.integers(0, k, G)
            pos[b, c, -1] = k - 1
    pos[B - 1, Nc - 1] = -1
    return pc, cand, pos


GATHER_F_V4 = (4, 20, 256, 260, 512, 1024)
GATHER_F_SCALAR = (1, 3, 50, 257)
GATHER_G = (1, 3, 4, 15, 16, 17, 33, 100)
GATHER_R = (1, 5)


def tail_start(G):
    """First position of the last chunk of 16 group members (the chunk gather_max_v4_kernel pads with skipped ids)."""
    return (G - 1) // 16 * 16


def gather_case(F, G, R, seed, num_rows=37):
    """-> feat (num_rows,F) float32, rows (R,G) int64.  Row r carries ids outside [0, num_rows) at the first position, the
    last and the middle of the tail chunk: below 0 / above / below for even r + seed, the other way round for odd (G < 4: at
    one of the three, in turn).  With R = 5, group 3 holds nothing but such ids and group 4 none (G = 1: every even group is all
    skipped)."""
    rng = np.random.default_rng(seed)
    feat = rng.standard_normal((num_rows, F)).astype(f32)
    rows = rng.integers(0, num_rows, (R, G)).astype(np.int64)
    below = lambda: -1 - int(rng.integers(0, 2 * num_rows))
    above = lambda: num_rows + int(rng.integers(0, 2 * num_rows))
    t0 = tail_start(G)
    for r in range(R):
        if r == 4 or (G == 1 and r % 2):
            continue
        if r == 3:
            rows[r] = [below() if rng.integers(0, 2) else above() for _ in range(G)]
            continue
        a, b = (below, above) if (r + seed) % 2 == 0 else (above, below)
        if G < 4:               # too short for three of them beside a valid id: one position per group
            rows[r, (0, G - 1, (G - 1) // 2)[r % 3]] = a()
            continue
        rows[r, t0 + (G - 1 - t0) // 2] = a()
        rows[r, G - 1] = b()
        rows[r, 0] = a()
    return feat, rows


def scene_case(F, G, seed, B=3, per_scene=4, scene_stride=50, used=30):
    """-> feat (B * scene_stride, F), index (B * per_scene, G) int64 LOCAL ids in [0, used) with skipped ids (-1, and one that
    lands behind the last feature row) at the first, last and a tail-chunk position, row_ids: a shuffled subset of the lists."""
    rng = np.random.default_rng(seed)
    num_rows = B * scene_stride
    feat = rng.standard_normal((num_rows, F)).astype(f32)
    index = rng.integers(0, used, (B * per_scene, G)).astype(np.int64)
    t0 = tail_start(G)
    for r in range(index.shape[0]):
        if r % 3 == 2:
            continue
        a, b = (-1 - r, num_rows + r) if r % 3 == 0 else (num_rows + r, -1 - r)
        if G < 4:
            index[r, (0, G - 1, (G - 1) // 2)[(r // 3) % 3]] = a
            continue
        index[r, t0 + (G - 1 - t0) // 2] = a
        index[r, G - 1] = b
        index[r, 0] = a
    row_ids = rng.permutation(B * per_scene)[:7].astype(np.int64)
    return feat, index, row_ids, per_scene, scene_stride


ARG_SHAPES = ((3, 5, 64), (64, 17, 40), (300, 4, 7), (256, 1, 3), (5, 100, 64))     # (F, G, R), R <= 64


def arg_case(F, G, R, seed, B=2, N=9):
    """-> feat (B N, F) float32 of the four values -1, 0, 1, 2 (different rows tie on most channels), rows (R,G) int64 with ids
    counting from the end, ids outside [-B N, B N) and, for R >= 3, group 2 made of those only; dy (R,F) float32 integers in
    [-4, 4]."""
    rng = np.random.default_rng(seed)
    num_rows = B * N
    feat = rng.integers(-1, 3, (num_rows, F)).astype(f32)
    rows = rng.integers(0, num_rows, (R, G)).astype(np.int64)
    kind = rng.integers(0, 8, (R, G))
    rows = np.where(kind == 0, rows - num_rows, rows)                                   # the same row, counted from the end
    rows = np.where(kind == 1, num_rows + rng.integers(0, 5, (R, G)), rows)             # skipped
    rows = np.where(kind == 2, -num_rows - 1 - rng.integers(0, 5, (R, G)), rows)        # skipped
    if R >= 3:
        rows[2] = np.where(rng.integers(0, 2, G) == 0, num_rows + 3, -num_rows - 2)
    dy = rng.integers(-4, 5, (R, F)).astype(f32)
    return feat, rows, dy, B, N


ROWSUM_K = (4, 8, 16, 32, 64, 128, 256)
ROWSUM_ROWS = (1, 2, 63, 64, 65, 1000)


def rowsum_case(kind, rows, K, seed):
    """kind integer: whole numbers in [-8, 8] (every partial sum is exact in float32); kind randn: standard normal."""
    rng = np.random.default_rng(seed)
    if kind == "integer":
        return rng.integers(-8, 9, (rows, K)).astype(f32)
    return rng.standard_normal((rows, K)).astype(f32)


def rowsum_bound(x):
    """Per row (K - 1) 2^-24 sum|x|: the worst case of a float32 sum of K terms in ANY order (every one of the K - 1 additions
    rounds a partial sum no larger than sum|x| by at most half an ulp)."""
    x = np.asarray(x, dtype=np.float64)
    return (x.shape[-1] - 1) * 2.0 ** -24 * np.abs(x).sum(axis=-1)
