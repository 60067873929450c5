"""numpy restatement of the multi-view fusion contract (DESIGN.md par. 5, include/regnet_hip.h), written from the contract text
and not from csrc/fuse.hip: the pose and the voxel coordinate in float32 arithmetic step by step (every array operation below is
on float32 arrays with float32 scalars, which numpy rounds one at a time), a dict keyed by the voxel key, Python-int sums, the
float64 finalise.  ``two_view_scene`` renders ``depth_reference``'s synthetic scene from two camera poses.
"""
import numpy as np

from . import depth_reference, plane_reference

f32 = np.float32
BIAS = 1 << 20
EMPTY = (1 << 64) - 1
HASH = 0x9E3779B97F4A7C15
QNAN = np.array([0x7FC00000], dtype=np.uint32).view(np.float32)[0]
DEFAULTS = {"voxel": 0.002, "origin": (0.0, 0.0, 0.0), "max_voxels": 1 << 20, "min_count": 1}


def pose12(pose):
    """Rows 0..2 of a 4x4 (None: identity), each entry rounded once to float32."""
    T = np.eye(4) if pose is None else np.asarray(pose, dtype=np.float64)
    return T[:3, :].reshape(12).astype(np.float32)


def inverse_voxel(voxel):
    """float32(1.0 / voxel), the division in float64."""
    return f32(1.0 / float(voxel))


def table_slots(max_voxels):
    p = 1
    while p < max_voxels:
        p *= 2
    return 2 * p


def workspace_bytes(max_voxels):
    """64 bytes of counters, 92 per slot, 4 per voxel, rounded up to 16."""
    return (64 + 92 * table_slots(max_voxels) + 4 * max_voxels + 15) // 16 * 16


def voxel_coords(xyz, pose, origin, inv):
    """(n,3) float32 rows -> (p (n,3) float32 transformed, i (n,3) int64, f (n,3) float32, finite (n), inside (n))."""
    xyz = np.asarray(xyz, dtype=np.float32).reshape(-1, 3)
    r = np.asarray(pose, dtype=np.float32)
    o = np.asarray(origin, dtype=np.float32)
    inv = f32(inv)
    x, y, z = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    with np.errstate(all="ignore"):
        p = np.stack([((r[4 * k] * x + r[4 * k + 1] * y) + r[4 * k + 2] * z) + r[4 * k + 3] for k in range(3)], axis=1)
        a = (p - o[None, :]) * inv
        fl = np.floor(a)
        ok = np.isfinite(a) & (fl >= f32(-BIAS)) & (fl < f32(BIAS))
        f = a - fl
    finite = np.isfinite(xyz).all(axis=1)
    inside = finite & ok.all(axis=1)
    i = np.where(ok, fl, 0).astype(np.int64)
    assert p.dtype == np.float32 and f.dtype == np.float32
    return p, i, f, finite, inside


def key_of(i):
    """Voxel coordinates (three ints in [-2^20, 2^20)) -> the 63-bit key."""
    return ((int(i[0]) + BIAS) << 42) | ((int(i[1]) + BIAS) << 21) | (int(i[2]) + BIAS)


def key(x, y, z, pose, origin, inv):
    """The key of one point, or None for a non-finite or out-of-range one."""
    _, i, _, _, inside = voxel_coords(np.array([[x, y, z]], dtype=np.float32), pose, origin, inv)
    return key_of(i[0]) if inside[0] else None


def home_slot(key, slots):
    """The top log2(slots) bits of key * HASH mod 2^64."""
    bits = slots.bit_length() - 1
    assert slots == 1 << bits and bits >= 1
    return ((int(key) * HASH) & EMPTY) >> (64 - bits)


def colour_level(c):
    """(int32)rintf(clamp(c, 0, 1) * 255.0f); NaN and everything not above 0 counts as 0."""
    c = np.asarray(c, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        pos = c > 0
        level = np.rint(np.minimum(np.where(pos, c, f32(0)), f32(1)) * f32(255))
    return np.where(pos, level, 0).astype(np.int64)


def _params(params):
    p = dict(DEFAULTS)
    if params is not None:
        p.update(params if isinstance(params, dict) else {k: getattr(params, k) for k in DEFAULTS})
    return p


def merge(clouds, poses=None, params=None):
    """The whole contract -> dict of ``xyz``, ``rgb`` (max_voxels,3) float32, ``count``, ``views``, ``first`` (max_voxels) int32,
    ``num`` (4) int32 and ``K``.  With more voxels than ``max_voxels`` only ``num[3] == 1`` is meaningful."""
    p = _params(params)
    mv, min_count = int(p["max_voxels"]), int(p["min_count"])
    origin = np.asarray(p["origin"], dtype=np.float64).astype(np.float32)
    inv = inverse_voxel(p["voxel"])
    poses = [None] * len(clouds) if poses is None else poses
    assert 1 <= len(clouds) <= 8 and len(poses) == len(clouds)
    table, offset, dropped, merged = {}, 0, 0, 0
    for v, ((xyz, rgb), pose) in enumerate(zip(clouds, poses)):
        xyz = np.asarray(xyz, dtype=np.float32).reshape(-1, 3)
        rgb = np.zeros_like(xyz) if rgb is None else np.asarray(rgb, dtype=np.float32).reshape(-1, 3)
        pt, i, f, _, inside = voxel_coords(xyz, pose12(pose), origin, inv)
        # an exact product, below 2^24 (2^24 where f was rounded up to 1)
        q = (np.where(inside[:, None], f, f32(0)) * f32(16777216.0)).astype(np.int64)
        level = colour_level(rgb)
        dropped += int((~inside).sum())
        for r in np.nonzero(inside)[0]:
            k = key_of(i[r])
            slot = table.get(k)
            if slot is None:
                slot = table[k] = {"count": 0, "S": [0, 0, 0], "C": [0, 0, 0], "first": offset + int(r), "views": 0, "i": i[r]}
            if slot["count"] == 0 or offset + int(r) <= slot["first"]:
                slot["first"], slot["point"], slot["colour"] = offset + int(r), pt[r].copy(), rgb[r].copy()
            slot["count"] += 1
            slot["views"] |= 1 << v
            for a in range(3):
                slot["S"][a] += int(q[r, a])
                slot["C"][a] += int(level[r, a])
            merged += 1
        offset += len(xyz)
    out = {"xyz": np.full((mv, 3), QNAN, dtype=np.float32), "rgb": np.zeros((mv, 3), dtype=np.float32),
           "count": np.full((mv,), -1, dtype=np.int32), "views": np.full((mv,), -1, dtype=np.int32),
           "first": np.full((mv,), -1, dtype=np.int32)}
    overflow = len(table) > mv
    kept = sorted(k for k, slot in table.items() if slot["count"] >= min_count)
    if overflow:
        kept = []
    inv64, o64 = float(inv), origin.astype(np.float64)
    for row, k in enumerate(kept):
        slot = table[k]
        n = slot["count"]
        if n == 1:
            out["xyz"][row], out["rgb"][row] = slot["point"], slot["colour"]
        else:
            for a in range(3):
                a_mean = float(slot["i"][a]) + float(slot["S"][a]) / (float(n) * 16777216.0)
                out["xyz"][row, a] = f32(o64[a] + a_mean / inv64)
                out["rgb"][row, a] = f32(float(slot["C"][a]) / (float(n) * 255.0))
        out["count"][row], out["views"][row], out["first"][row] = n, slot["views"], slot["first"]
    out["num"] = np.array([len(kept), merged, dropped, int(overflow)], dtype=np.int32)
    out["K"] = len(kept)
    return out


TWO_VIEW_VOXEL = 0.05     # merged at this voxel, two_view_scene()'s default frames occupy
TWO_VIEW_K = 1953         # ... so many voxels (found with merge() alone), 998 of them seen by both cameras


CAMERAS = ((0.0, 0.0, 0.0), (0.3, 0.0, 12.0), (-0.3, 0.0, -12.0), (0.0, 0.25, 8.0))   # moved by (x, y) [m], turned about z [deg]


def two_view_scene(width=64, height=48, seed=5, views=2):
    """``views`` (up to 4) depth images of ``depth_reference``'s scene: the default camera, one moved 0.3 m along the table's x and
    turned 12 degrees about the table's z, and so on down ``CAMERAS``.  -> (frames, poses): per view the ``DepthFrame`` keywords
    (uint16 depth, aligned colour) and the 4x4 camera-to-common transform, the common frame being the first camera's."""
    rng = np.random.RandomState(seed)
    scale = width / 640.0
    K = (460.0 * scale, 460.0 * scale, (width - 1) / 2.0, (height - 1) / 2.0)
    first = plane_reference.default_transform()                      # camera 0 -> table
    frames, poses = [], []
    for dx, dy, degrees in CAMERAS[:views]:
        turn = np.eye(4)
        a = np.radians(degrees)
        turn[:2, :2] = [[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]]
        turn[:3, 3] = [dx, dy, 0.0]
        to_table = turn @ first                                      # this camera -> table
        truth, ids = depth_reference.ray_cast(width, height, K, to_table)
        raw = np.clip(np.rint(truth * 1000.0), 0, 65535).astype(np.uint16)
        colour = np.clip(depth_reference.PALETTE[np.maximum(ids, 0)] + rng.randint(-25, 26, size=ids.shape + (3,)), 0, 255)
        frames.append({"depth": raw, "intrinsics": K, "color": colour.astype(np.uint8), "depth_scale": 0.001})
        poses.append(np.linalg.inv(first) @ to_table)
    return frames, poses
