"""Object segmentation restated in numpy float32, from the contract alone (include/regnet_hip.h, DESIGN.md par. 5, "object
segmentation"): individually rounded binary32 operations in the written order.  numpy rounds every float32 operation on its own
(there is no contraction), for scalars and element-wise over arrays alike.  Nothing here imports the package's kernels.

  graph rows  mask (or all rows) and three finite coordinates
  edges       d2 = ((dx dx) + (dy dy)) + (dz dz) <= T2, dx = x_i - x_j, T2 = float32(t) * float32(t)      (inclusive)
  root        the smallest row of the row's connected component, -1 outside the graph
  ranking     components of size >= min_points, by descending size, equal sizes by smaller root; rank r < max_objects = object r
  label       the object id or -1;  num = (min(kept, max_objects), kept)
  tables      size, first (= root) and bbox (min x, y, z, max x, y, z; -0.0 < +0.0) of every object, -1 / -1 / NaN beyond
  assign      the row with label >= 0 and d2 <= R2 that is smallest by (d2, row); its label; -1 / -1 without one
"""
import numpy as np

f32 = np.float32
BLOCK = 512


def sqdist(a, b):
    """(n,3), (m,3) float32 -> (n,m) float32: ((dx dx) + (dy dy)) + (dz dz) with dx = a - b."""
    a, b = np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        dx = a[:, None, 0] - b[None, :, 0]
        dy = a[:, None, 1] - b[None, :, 1]
        dz = a[:, None, 2] - b[None, :, 2]
        return (dx * dx + dy * dy) + dz * dz


def graph_rows(xyz, mask=None):
    xyz = np.asarray(xyz, dtype=np.float32).reshape(-1, 3)
    ok = np.isfinite(xyz).all(axis=1)
    if mask is not None:
        ok &= np.asarray(mask).reshape(-1) != 0
    return ok


def edges(xyz, rows, tolerance):
    """The pairs (i, j), i < j, of graph rows with d2 <= T2: blocked all-pairs."""
    t = f32(tolerance)
    T2 = f32(t * t)
    xyz = np.asarray(xyz, dtype=np.float32)
    out = []
    for a in range(0, len(rows), BLOCK):
        ra = rows[a:a + BLOCK]
        for b in range(a, len(rows), BLOCK):
            rb = rows[b:b + BLOCK]
            close = sqdist(xyz[ra], xyz[rb]) <= T2
            ia, ib = np.nonzero(close)
            i, j = ra[ia], rb[ib]
            out.append(np.stack([i[i < j], j[i < j]], axis=1))
    return np.concatenate(out) if out else np.zeros((0, 2), dtype=np.int64)


def components(n, pairs):
    """A plain union-find over rows 0..n-1 -> root (n): the smallest row of every row's component."""
    parent = list(range(n))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    for i, j in pairs:
        a, b = find(int(i)), find(int(j))
        if a != b:
            parent[max(a, b)] = min(a, b)
    return np.array([find(x) for x in range(n)], dtype=np.int64)


def _ordered(v):
    """float32 -> uint32 keys that order like the values, with -0.0 below +0.0."""
    u = np.asarray(v, dtype=np.float32).view(np.uint32)
    return np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000))


def cluster_points(xyz, mask=None, tolerance=0.01, min_points=50, max_objects=64):
    """-> dict: root, label (n) int32; num (2) int32; size, first (max_objects) int32; bbox (max_objects, 6) float32."""
    xyz = np.ascontiguousarray(np.asarray(xyz, dtype=np.float32).reshape(-1, 3))
    n = len(xyz)
    ok = graph_rows(xyz, mask)
    rows = np.nonzero(ok)[0]
    root = np.full((n,), -1, dtype=np.int32)
    root[rows] = components(n, edges(xyz, rows, tolerance))[rows]
    roots, sizes = np.unique(root[rows], return_counts=True)            # ascending root
    keep = sizes >= min_points
    roots, sizes = roots[keep], sizes[keep]
    rank = np.argsort(-sizes, kind="stable")                            # descending size, equal sizes by smaller root
    roots, sizes = roots[rank], sizes[rank]
    kept = len(roots)
    count = min(kept, max_objects)
    label = np.full((n,), -1, dtype=np.int32)
    size = np.full((max_objects,), -1, dtype=np.int32)
    first = np.full((max_objects,), -1, dtype=np.int32)
    bbox = np.full((max_objects, 6), np.nan, dtype=np.float32)
    for obj in range(count):
        members = root == roots[obj]
        label[members] = obj
        size[obj], first[obj] = sizes[obj], roots[obj]
        pts = xyz[members]
        keys = _ordered(pts)
        for a in range(3):
            bbox[obj, a] = pts[np.argmin(keys[:, a]), a]
            bbox[obj, 3 + a] = pts[np.argmax(keys[:, a]), a]
    return {"root": root, "label": label, "num": np.array([count, kept], dtype=np.int32), "size": size, "first": first,
            "bbox": bbox}


def assign(query, xyz, label, radius):
    """-> (object (q) int32, point (q) int32)."""
    query = np.asarray(query, dtype=np.float32).reshape(-1, 3)
    xyz = np.asarray(xyz, dtype=np.float32).reshape(-1, 3)
    label = np.asarray(label).reshape(-1)
    r = f32(radius)
    R2 = f32(r * r)
    obj = np.full((len(query),), -1, dtype=np.int32)
    point = np.full((len(query),), -1, dtype=np.int32)
    rows = np.nonzero(label >= 0)[0]
    for a in range(0, len(query), BLOCK):
        q = query[a:a + BLOCK]
        d2 = sqdist(q, xyz[rows])
        with np.errstate(invalid="ignore"):
            ok = (d2 <= R2) & np.isfinite(q).all(axis=1)[:, None]
        d2 = np.where(ok, d2, np.inf)
        for k in range(len(q)):
            if ok[k].any():
                best = rows[np.nonzero(ok[k] & (d2[k] == d2[k].min()))[0][0]]      # the lowest row among the nearest
                point[a + k], obj[a + k] = best, label[best]
    return obj, point


def above_table_mask(points32, table_height, clearance):
    level = f32(f32(table_height) + f32(clearance))
    return np.asarray(points32, dtype=np.float32)[:, 2] > level


def select_per_object(keep, object, num_objects, k):
    """``keep``: the rows pose NMS kept, in rank order; ``object`` (n): every row's object.  -> (index, object_of_row): the
    first ``k`` kept rows of each object id in [0, num_objects), by object id, then by rank."""
    object = np.asarray(object).reshape(-1)
    index, objects = [], []
    for obj in range(int(num_objects)):
        mine = [int(r) for r in keep if object[int(r)] == obj][:int(k)]
        index += mine
        objects += [obj] * len(mine)
    return np.array(index, dtype=np.int64), np.array(objects, dtype=np.int32)


# ---- test inputs ----------------------------------------------------------------------------------------------------------
def blobs(seed, n, clusters=5, spread=0.008, noise=0.2, extent=0.25):
    """Seeded Gaussian blobs plus uniform noise, shuffled -> (n,3) float32."""
    rng = np.random.RandomState(seed)
    centres = rng.uniform(-extent, extent, (max(clusters, 1), 3))
    member = rng.randint(0, max(clusters, 1), n)
    pts = centres[member] + rng.normal(0.0, spread, (n, 3))
    lone = rng.rand(n) < noise
    pts[lone] = rng.uniform(-extent * 1.5, extent * 1.5, (int(lone.sum()), 3))
    return np.ascontiguousarray(pts.astype(np.float32))


def snake(seed, n, step=0.004):
    """One component joined only through consecutive neighbours (a helix whose turns are 5 steps apart), in shuffled row order
    -> (xyz (n,3) float32, tolerance)."""
    s = np.arange(n) * step
    radius = 0.05
    theta = s / radius
    pts = np.stack([radius * np.cos(theta), radius * np.sin(theta), s * (5 * step / (2 * np.pi * radius))], axis=1)
    return np.ascontiguousarray(pts[np.random.RandomState(seed).permutation(n)].astype(np.float32)), 1.5 * step


def lattice(shape=(3, 3, 2), spacing=0.5):
    """Points on a lattice whose spacing is an exact binary fraction -> (n,3) float32."""
    g = np.stack(np.meshgrid(*[np.arange(s) for s in shape], indexing="ij"), axis=-1).reshape(-1, 3)
    return np.ascontiguousarray((g * spacing).astype(np.float32))
