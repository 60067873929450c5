"""numpy restatement of the depth-frame contract (DESIGN.md par. 5, include/regnet_hip.h), written from the contract text and not
from csrc/depth.hip: depth decoding and range, the one-pass edge filter, the division-free deprojection, the three colour modes
with the colour camera's z-buffer, the status codes and their histogram.  Every array operation below is on float32 arrays with
float32 scalars: numpy rounds each on its own (no fused multiply-add), which is what the contract asks of the kernels.
``synthetic_depth_frame`` ray-casts the scene of ``plane_reference.synthetic_frame`` into what a depth camera delivers.
"""
import math
from types import SimpleNamespace

import numpy as np

from . import plane_reference

f32 = np.float32
QNAN_BITS = 0x7FC00000
NO_DEPTH, OUT_OF_RANGE, EDGE_JUMP, FEW_NEIGHBOURS, OUTSIDE, OCCLUDED, KEPT = range(7)
NEIGHBOURS = [(dy, dx) for dy in (-1, 0, 1) for dx in (-1, 0, 1) if (dy, dx) != (0, 0)]


def lut():
    """LUT[i] = float32(i / 255.0): the division in float64, rounded once."""
    return (np.arange(256, dtype=np.float64) / 255.0).astype(np.float32)


def reciprocal(f):
    """float32(1 / float64(f))."""
    return f32(1.0 / float(f))


def depth_metres(depth, depth_scale=0.001):
    """-> (z (H,W) float32, has (H,W) bool).  uint16 d: z = float32(d) * s, d == 0 no depth; float32: z = d, a non-finite z or
    z <= 0 no depth."""
    depth = np.asarray(depth)
    if depth.dtype == np.uint16:
        with np.errstate(over="ignore"):
            return depth.astype(np.float32) * f32(depth_scale), depth != 0
    z = depth.astype(np.float32)
    with np.errstate(invalid="ignore"):
        return z, np.isfinite(z) & (z > 0)


def valid0(z, has, lo=0.0, hi=math.inf):
    """has depth and lo <= z <= hi, inclusive, in float32."""
    with np.errstate(invalid="ignore"):
        return has & (f32(lo) <= z) & (z <= f32(hi))


def shifted(a, dy, dx, fill):
    """b[v, u] = a[v + dy, u + dx], ``fill`` beyond the image."""
    H, W = a.shape
    out = np.full_like(a, fill)
    vs, us = slice(max(0, -dy), min(H, H - dy)), slice(max(0, -dx), min(W, W - dx))
    vq, uq = slice(max(0, dy), min(H, H + dy)), slice(max(0, dx), min(W, W + dx))
    out[vs, us] = a[vq, uq]
    return out


def edge_filter(z, valid, t):
    """-> (jump (H,W) bool, neighbours (H,W) int): for a valid0 pixel, over its 8 neighbours inside the image that are valid0:
    jump when fabsf(z - zq) > t * fminf(z, zq) (strict); the count of such neighbours.  ``t`` None: no jump anywhere."""
    jump = np.zeros(z.shape, dtype=bool)
    neighbours = np.zeros(z.shape, dtype=np.int32)
    for dy, dx in NEIGHBOURS:
        vq = shifted(valid, dy, dx, False)
        neighbours += vq
        if t is not None:
            zq = shifted(z, dy, dx, f32(0))
            with np.errstate(invalid="ignore", over="ignore"):
                e = f32(t) * np.minimum(z, zq)
                jump |= valid & vq & (np.abs(z - zq) > e)
    return jump, neighbours


def deproject(z, intrinsics):
    """x = ((float32(u) - cx) * z) * rfx, y likewise, z: (H,W,3) float32."""
    fx, fy, cx, cy = intrinsics
    H, W = z.shape
    u = np.arange(W, dtype=np.float32)[None, :]
    v = np.arange(H, dtype=np.float32)[:, None]
    with np.errstate(invalid="ignore", over="ignore"):
        x = ((u - f32(cx)) * z) * reciprocal(fx)
        y = ((v - f32(cy)) * z) * reciprocal(fy)
    return np.stack([x, y, z.astype(np.float32)], axis=-1)


def project(xyz, depth_to_color, color_intrinsics, Wc, Hc):
    """-> (inside bool, fu int, fv int, zp float32) for (..., 3) float32 points: p' = R p + t in the written order, outside when
    z' is not finite or <= 0, uc = (x' / z') * fxc + cxc, fu = floorf(uc + 0.5), inside when 0 <= fu < Wc in float; fv alike."""
    T = np.asarray(depth_to_color, dtype=np.float64).astype(np.float32)
    fxc, fyc, cxc, cyc = (f32(c) for c in color_intrinsics)
    x, y, z = xyz[..., 0], xyz[..., 1], xyz[..., 2]
    with np.errstate(all="ignore"):
        row = lambda i: ((T[i, 0] * x + T[i, 1] * y) + T[i, 2] * z) + T[i, 3]      # noqa: E731
        xp, yp, zp = row(0), row(1), row(2)
        ok = np.isfinite(zp) & (zp > 0)
        uc = (xp / zp) * fxc + cxc
        vc = (yp / zp) * fyc + cyc
        fu, fv = np.floor(uc + f32(0.5)), np.floor(vc + f32(0.5))
        inside = ok & (fu >= 0) & (fu < f32(Wc)) & (fv >= 0) & (fv < f32(Hc))
    fu = np.where(inside, fu, 0).astype(np.int64)
    fv = np.where(inside, fv, 0).astype(np.int64)
    return inside, fu, fv, zp


def z_buffer(inside, fu, fv, zp, Wc, Hc, splat):
    """(Hc, Wc) float32: +inf, then the minimum z' over every inside point's (2 splat + 1)^2 footprint clipped to the image."""
    zb = np.full((Hc * Wc,), np.inf, dtype=np.float32)
    fu, fv, zp = fu[inside], fv[inside], zp[inside]
    for dy in range(-splat, splat + 1):
        for dx in range(-splat, splat + 1):
            uu, vv = fu + dx, fv + dy
            m = (uu >= 0) & (uu < Wc) & (vv >= 0) & (vv < Hc)
            np.minimum.at(zb, vv[m] * Wc + uu[m], zp[m])
    return zb.reshape(Hc, Wc)


def to_cloud(depth, intrinsics, color=None, color_intrinsics=None, depth_to_color=None, depth_scale=0.001,
             depth_range=(0.0, math.inf), edge_threshold=None, min_neighbours=0, occlusion_margin=0.01, splat=1,
             keep_uncoloured=False, details=False):
    """The whole contract -> (xyz (H W,3) float32, rgb (H W,3) float32, status (H W) uint8, counts (8) int32)."""
    z, has = depth_metres(depth, depth_scale)
    H, W = z.shape
    valid = valid0(z, has, *depth_range)
    status = np.where(has, OUT_OF_RANGE, NO_DEPTH).astype(np.uint8)
    jump, neighbours = edge_filter(z, valid, edge_threshold)
    survive = valid & ~jump & (neighbours >= min_neighbours)
    status[valid & jump] = EDGE_JUMP
    status[valid & ~jump & (neighbours < min_neighbours)] = FEW_NEIGHBOURS
    status[survive] = KEPT
    pts = deproject(z, intrinsics)
    rgb = np.zeros((H, W, 3), dtype=np.float32)
    keep_xyz = survive.copy()
    extra = None
    if color is not None and color_intrinsics is None:
        color = np.asarray(color)
        assert color.shape == (H, W, 3) and color.dtype == np.uint8
        rgb[survive] = lut()[color[survive]]
    elif color is not None:
        color = np.asarray(color)
        Hc, Wc = color.shape[:2]
        inside, fu, fv, zp = project(pts, depth_to_color, color_intrinsics, Wc, Hc)
        inside &= survive
        zb = z_buffer(inside, fu, fv, zp, Wc, Hc, splat)
        with np.errstate(invalid="ignore"):
            visible = inside & ((zp - zb[fv, fu]) <= f32(occlusion_margin))
        status[survive & ~inside] = OUTSIDE
        status[inside & ~visible] = OCCLUDED
        rgb[visible] = lut()[color[fv[visible], fu[visible]]]
        if not keep_uncoloured:
            keep_xyz = visible
        extra = SimpleNamespace(inside=inside, visible=visible, fu=fu, fv=fv, zp=zp, zbuffer=zb)
    xyz = np.where(keep_xyz[..., None], pts, np.array([QNAN_BITS], dtype=np.uint32).view(np.float32)[0]).astype(np.float32)
    status = status.reshape(-1)
    counts = np.bincount(status, minlength=8).astype(np.int32)
    out = (np.ascontiguousarray(xyz.reshape(-1, 3)), np.ascontiguousarray(rgb.reshape(-1, 3)), status, counts)
    return out + (extra,) if details else out


def frame_kwargs(frame, registered=False, aligned=False):
    """The synthetic frame as ``to_cloud``'s (and ``DepthFrame``'s) keywords in one of the three colour modes."""
    kw = {"depth": frame.depth, "intrinsics": frame.intrinsics, "depth_scale": frame.depth_scale}
    if aligned:
        kw["color"] = frame.color_aligned
    if registered:
        kw.update(color=frame.color, color_intrinsics=frame.color_intrinsics, depth_to_color=frame.depth_to_color)
    return kw


# ---- the synthetic depth camera -------------------------------------------------------------------------------------------------
# the scene of plane_reference.synthetic_frame as solids in the table frame: (lo, hi) corners; the floor is the plane z = 0
TABLE = ((-0.6, 0.0, 0.0), (0.5, 0.9, 0.75))
BOXES = [((cx - h, cy - h, 0.75), (cx + h, cy + h, 0.75 + tall))
         for cx, cy, h, tall in ((-0.1, 0.4, 0.06, 0.1), (0.1, 0.5, 0.05, 0.15), (-0.2, 0.3, 0.08, 0.05), (0.0, 0.3, 0.04, 0.2))]
PALETTE = np.array([[90, 80, 70], [170, 120, 60], [200, 40, 40], [40, 180, 60], [50, 70, 210], [220, 200, 40]], dtype=np.int64)


def ray_cast(width, height, intrinsics, camera_to_table):
    """Per pixel the first surface along its ray: -> (depth (H,W) float64 = the camera-frame z of the hit, 0 for no hit;
    ids (H,W) int: 0 floor, 1 table, 2..5 the boxes, -1 nothing).  Slab tests against the axis-aligned solids."""
    fx, fy, cx, cy = intrinsics
    T = np.asarray(camera_to_table, dtype=np.float64)
    u, v = np.meshgrid(np.arange(width, dtype=np.float64), np.arange(height, dtype=np.float64))
    d = np.stack([(u - cx) / fx, (v - cy) / fy, np.ones_like(u)], axis=-1) @ T[:3, :3].T       # z component 1 in the camera
    o = T[:3, 3]
    best = np.full((height, width), np.inf)
    ids = np.full((height, width), -1, dtype=np.int64)
    with np.errstate(divide="ignore", invalid="ignore"):
        t = -o[2] / d[..., 2]                                                               # the floor
        hit = (d[..., 2] < 0) & (t > 0)
        best[hit], ids[hit] = t[hit], 0
        for k, (lo, hi) in enumerate([TABLE] + BOXES):
            t1 = (np.asarray(lo) - o) / d
            t2 = (np.asarray(hi) - o) / d
            near, far = np.minimum(t1, t2).max(axis=-1), np.maximum(t1, t2).min(axis=-1)
            hit = (far >= near) & (near > 0) & (near < best)
            best[hit], ids[hit] = near[hit], k + 1
    return np.where(np.isfinite(best), best, 0.0), ids


def synthetic_depth_frame(seed=5, width=640, height=480, noise=0.0015, holes=0.05, mixed=0.5, baseline=0.04):
    """A seeded depth-camera frame of ``plane_reference.synthetic_frame``'s scene from the default camera pose:

    ``depth`` (H,W) uint16 millimetres with ``noise`` [m] Gaussian noise and a share ``holes`` of zero pixels; at a share ``mixed``
    of the silhouette pixels (a 4-neighbour shows another surface more than 2 cm away in depth) the depth is the mean of the near
    and the far depth (``is_mixed``); ``color_aligned`` (H,W,3) uint8 on the depth grid; ``color`` (Hc,Wc,3) uint8 of a second
    camera with its own intrinsics, 1.25 x the resolution, ``baseline`` metres to the side and slightly turned
    (``color_intrinsics``, ``depth_to_color``); ``ids`` / ``color_ids``: the surface each camera's ray hits."""
    rng = np.random.RandomState(seed)
    scale = width / 640.0
    K = (460.0 * scale, 460.0 * scale, (width - 1) / 2.0, (height - 1) / 2.0)
    pose = plane_reference.default_transform()
    truth, ids = ray_cast(width, height, K, pose)
    depth = truth.copy()
    is_mixed = np.zeros((height, width), dtype=bool)
    for dy, dx in ((0, 1), (0, -1), (1, 0), (-1, 0)):
        other, other_id = shifted(truth, dy, dx, 0.0), shifted(ids, dy, dx, -1)
        edge = (other_id != ids) & (other_id >= 0) & (ids >= 0) & (np.abs(other - truth) > 0.02) & ~is_mixed
        pick = edge & (rng.rand(height, width) < mixed / 2.0)          # (a silhouette pixel usually has two such neighbours)
        depth[pick] = 0.5 * (truth[pick] + other[pick])
        is_mixed |= pick
    depth = depth + rng.normal(0.0, noise, depth.shape) * (truth > 0)
    raw = np.clip(np.rint(depth * 1000.0), 0, 65535).astype(np.uint16)
    raw[rng.rand(height, width) < holes] = 0
    is_mixed &= raw != 0

    def paint(surface):
        c = PALETTE[np.maximum(surface, 0)] + rng.randint(-25, 26, size=surface.shape + (3,))
        return np.clip(c, 0, 255).astype(np.uint8)
    color_aligned = paint(ids)
    Wc, Hc = int(round(width * 1.25)), int(round(height * 1.25))
    Kc = (560.0 * scale, 565.0 * scale, (Wc - 1) / 2.0 + 3.0, (Hc - 1) / 2.0 - 2.0)
    a = math.radians(1.5)
    D2C = np.eye(4)
    D2C[:3, :3] = [[math.cos(a), 0, math.sin(a)], [0, 1, 0], [-math.sin(a), 0, math.cos(a)]]
    D2C[:3, 3] = [-baseline, 0.004, 0.002]
    _, color_ids = ray_cast(Wc, Hc, Kc, pose @ np.linalg.inv(D2C))
    return SimpleNamespace(depth=raw, intrinsics=K, depth_scale=0.001, color_aligned=color_aligned, color=paint(color_ids),
                           color_intrinsics=Kc, depth_to_color=D2C, ids=ids, color_ids=color_ids, is_mixed=is_mixed, truth=truth)
