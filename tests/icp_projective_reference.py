"""numpy restatement of the projective mode of the pose refinement and of the normals of an organised cloud (include/regnet_hip.h,
DESIGN.md par. 5), written from the contract text and not from csrc/icp.hip or csrc/depth.hip: the projection, the window, the
normal gate and the differences of ``image_normals`` in float32 arithmetic step by step (every array operation on float32 arrays,
which numpy rounds one at a time; its division and square root are correctly rounded), ties to the lowest row.  Sums, solve,
update and the status rules are ``tests/icp_reference.py``'s, imported and not copied.  ``render`` is a small analytic renderer
of rectangles and a sphere into the organised cloud of a pinhole camera; ``corner_room`` is the scene the loop is tested on.
"""
import math

import numpy as np

from .icp_reference import (CONVERGED, DEFAULTS, DEGENERATE, MAX_ITER, RUNNING, TOO_FEW, cholesky_solve, max_dist2,  # noqa: F401
                            pose12, sums, system, transform, update)

f32 = np.float32
PROJECTIVE_DEFAULTS = dict(DEFAULTS, window=1, min_cos=None)


def project(p, intrinsics, width, height):
    """``p`` (n,3) float32 in the camera's frame -> (u, v, inside): the pixel a point falls on, int64, and whether there is one:
    p finite with p_z > 0, uf = (p_x / p_z) * fx + cx, fu = floor(uf + 0.5), 0 <= fu < W in float, likewise v."""
    p = np.asarray(p, dtype=np.float32).reshape(-1, 3)
    with np.errstate(over="ignore"):
        fx, fy, cx, cy = (f32(v) for v in intrinsics)
    with np.errstate(all="ignore"):
        ok = np.isfinite(p).all(axis=1) & (p[:, 2] > 0)
        uf = ((p[:, 0] / p[:, 2]) * fx) + cx
        vf = ((p[:, 1] / p[:, 2]) * fy) + cy
        fu, fv = np.floor(uf + f32(0.5)), np.floor(vf + f32(0.5))
        assert fu.dtype == fv.dtype == np.float32
        inside = ok & (fu >= 0) & (fu < f32(width)) & (fv >= 0) & (fv < f32(height))
    u = np.where(inside, fu, 0).astype(np.int64)
    v = np.where(inside, fv, 0).astype(np.int64)
    return u, v, inside


def rotate(normals, pose):
    """((r0 s_x) + (r1 s_y)) + (r2 s_z) per coordinate with the float32 rotation of ``pose12`` -> (n,3) float32."""
    s = np.asarray(normals, dtype=np.float32).reshape(-1, 3)
    r = pose12(pose)
    with np.errstate(all="ignore"):
        m = np.stack([((r[4 * k] * s[:, 0]) + (r[4 * k + 1] * s[:, 1])) + (r[4 * k + 2] * s[:, 2]) for k in range(3)], axis=1)
    assert m.dtype == np.float32
    return m


def correspond_projective(source, target, target_normals, width, height, intrinsics, pose, max_dist, stride=1, window=1,
                          source_normals=None, min_cos=None):
    """-> (idx (rows,) int32, p (rows,3) float32): per visited source row the accepted target row v W + u, -1 rejected, -2
    skipped.  ``min_cos`` None: the gate is off and ``source_normals`` is not looked at."""
    source = np.asarray(source, dtype=np.float32).reshape(-1, 3)[::int(stride)]
    target = np.asarray(target, dtype=np.float32).reshape(-1, 3)
    normals = np.asarray(target_normals, dtype=np.float32).reshape(-1, 3)
    assert len(target) == len(normals) == width * height
    p = transform(source, pose)
    n = len(source)
    idx = np.full((n,), -1, dtype=np.int32)
    skipped = ~np.isfinite(source).all(axis=1)
    u, v, inside = project(p, intrinsics, width, height)
    alive = inside & ~skipped
    if min_cos is not None:
        s = np.asarray(source_normals, dtype=np.float32).reshape(-1, 3)[::int(stride)]
        m = rotate(s, pose)
        alive &= np.isfinite(s).all(axis=1)
        with np.errstate(over="ignore"):
            c32 = f32(min_cos)
    usable = np.isfinite(target).all(axis=1) & np.isfinite(normals).all(axis=1)
    best = np.full((n,), np.inf, dtype=np.float32)
    row = np.full((n,), -1, dtype=np.int64)
    for b in range(-window, window + 1):                   # ascending rows: of equal d2 the first, the lowest row, stays
        for a in range(-window, window + 1):
            cu, cv = u + a, v + b
            ok = alive & (cu >= 0) & (cu < width) & (cv >= 0) & (cv < height)
            j = np.where(ok, cv * width + cu, 0)
            ok &= usable[j]
            q, nq = target[j], normals[j]
            with np.errstate(all="ignore"):
                if min_cos is not None:
                    dot = ((m[:, 0] * nq[:, 0]) + (m[:, 1] * nq[:, 1])) + (m[:, 2] * nq[:, 2])
                    assert dot.dtype == np.float32
                    ok &= dot >= c32
                d = p - q
                d2 = ((d[:, 0] * d[:, 0]) + (d[:, 1] * d[:, 1])) + (d[:, 2] * d[:, 2])
            assert d2.dtype == np.float32
            with np.errstate(invalid="ignore"):
                better = ok & (d2 < best)
            best = np.where(better, d2, best)
            row = np.where(better, j, row)
    accept = (row >= 0) & (best <= max_dist2(max_dist))
    idx[accept] = row[accept]
    idx[skipped] = -2
    return idx, p


def image_normals(xyz, width, height, step=2, max_jump=0.02):
    """The normals of an organised cloud -> (H W, 3) float32, NaN where a pixel has none."""
    W, H, step = int(width), int(height), int(step)
    c = np.asarray(xyz, dtype=np.float32).reshape(H, W, 3)
    with np.errstate(over="ignore"):
        jump = f32(max_jump)

    def shifted(du, dv):
        """The pixel (u + du, v + dv) at (u, v); NaN beyond the image."""
        out = np.full((H, W, 3), np.nan, dtype=np.float32)
        if abs(du) < W and abs(dv) < H:
            out[max(0, -dv):H - max(0, dv), max(0, -du):W - max(0, du)] = c[max(0, dv):H - max(0, -dv), max(0, du):W - max(0, -du)]
        return out

    def difference(du, dv):
        near, far = shifted(-du, -dv), shifted(du, dv)
        with np.errstate(all="ignore"):
            ok_near = np.isfinite(near).all(axis=2) & (np.abs(near[:, :, 2] - c[:, :, 2]) <= jump)
            ok_far = np.isfinite(far).all(axis=2) & (np.abs(far[:, :, 2] - c[:, :, 2]) <= jump)
            a = np.where(ok_near[:, :, None], near, c)
            b = np.where(ok_far[:, :, None], far, c)
            d = b - a
        assert d.dtype == np.float32
        return d, ok_near | ok_far

    h, has_h = difference(step, 0)
    g, has_g = difference(0, step)
    with np.errstate(all="ignore"):
        n = np.stack([(h[:, :, 1] * g[:, :, 2]) - (h[:, :, 2] * g[:, :, 1]), (h[:, :, 2] * g[:, :, 0]) - (h[:, :, 0] * g[:, :, 2]),
                      (h[:, :, 0] * g[:, :, 1]) - (h[:, :, 1] * g[:, :, 0])], axis=2)
        len2 = ((n[:, :, 0] * n[:, :, 0]) + (n[:, :, 1] * n[:, :, 1])) + (n[:, :, 2] * n[:, :, 2])
        ok = np.isfinite(c).all(axis=2) & has_h & has_g & np.isfinite(len2) & (len2 > 0)
        n = n / np.sqrt(len2)[:, :, None]
        dot = ((n[:, :, 0] * c[:, :, 0]) + (n[:, :, 1] * c[:, :, 1])) + (n[:, :, 2] * c[:, :, 2])
        n = np.where((dot > 0)[:, :, None], -n, n)
    assert n.dtype == np.float32 and len2.dtype == np.float32
    return np.where(ok[:, :, None], n, f32(np.nan)).reshape(H * W, 3)


def step_projective(source, target, target_normals, width, height, intrinsics, pose, params, iteration, source_normals=None):
    """One iteration -> (pose, status, pairs, rms, idx, sums): ``icp_reference.step`` with the projective correspondences."""
    idx, p = correspond_projective(source, target, target_normals, width, height, intrinsics, pose, params["max_dist"],
                                   params["stride"], params["window"], source_normals, params["min_cos"])
    s, _ = sums(p, target, target_normals, idx)
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


def icp_projective(source, target, target_normals, width, height, intrinsics, init=None, params=None, source_normals=None):
    """The loop -> ``icp_reference.icp``'s dict.  ``params``: ``icp_reference.DEFAULTS``' keys, ``window`` and ``min_cos``
    (None: the gate is off)."""
    p = dict(PROJECTIVE_DEFAULTS)
    p.update(params or {})
    pose = np.eye(4) if init is None else np.array(init, dtype=np.float64)
    history, status, it = [], RUNNING, 0
    while status == RUNNING:
        pose, status, pairs, rms, _, _ = step_projective(source, target, target_normals, width, height, intrinsics, pose, p, it,
                                                         source_normals)
        history.append((float(pairs), rms))
        it += 1
    history = np.array(history, dtype=np.float64).reshape(-1, 2)
    return {"pose": pose, "status": status, "iterations": it, "history": history, "pairs": int(history[-1, 0]),
            "rms_first": float(history[0, 1]), "rms_last": float(history[-1, 1])}


def min_cos(normal_angle):
    """``IcpParams.normal_angle`` [deg] or None -> the restatement's ``min_cos``."""
    return None if normal_angle is None else math.cos(math.radians(float(normal_angle)))


# ---- an analytic renderer ----------------------------------------------------------------------------------------------------
def rectangle(origin, edge_a, edge_b):
    """The parallelogram origin + s edge_a + t edge_b, 0 <= s, t <= 1."""
    return ("rectangle", np.asarray(origin, dtype=np.float64), np.asarray(edge_a, dtype=np.float64), np.asarray(edge_b, dtype=np.float64))


def sphere(centre, radius):
    return ("sphere", np.asarray(centre, dtype=np.float64), float(radius))


def render(scene, width, height, intrinsics, camera=None):
    """The organised cloud a pinhole camera at ``camera`` (4x4 camera-to-world, None: identity) sees of ``scene`` (a list of
    ``rectangle`` / ``sphere``), in the CAMERA's frame: per pixel (u, v) the ray ((u - cx) / fx, (v - cy) / fy, 1) t, its nearest
    hit with t > 0 in float64, rounded once to float32 -> (H W, 3) float32, NaN rows where the ray hits nothing."""
    fx, fy, cx, cy = (float(v) for v in intrinsics)
    T = np.eye(4) if camera is None else np.asarray(camera, dtype=np.float64)
    u, v = np.meshgrid(np.arange(width, dtype=np.float64), np.arange(height, dtype=np.float64))
    d_cam = np.stack([(u - cx) / fx, (v - cy) / fy, np.ones_like(u)], axis=2).reshape(-1, 3)
    d = d_cam @ T[:3, :3].T
    o = T[:3, 3]
    best = np.full((len(d),), np.inf)
    with np.errstate(all="ignore"):
        for item in scene:
            if item[0] == "rectangle":
                _, origin, ea, eb = item
                n = np.cross(ea, eb)
                t = ((origin - o) @ n) / (d @ n)
                hit = o[None, :] + t[:, None] * d - origin[None, :]
                s_a, s_b = (hit @ ea) / (ea @ ea), (hit @ eb) / (eb @ eb)       # (the edges are orthogonal in every scene here)
                ok = (t > 0) & (s_a >= 0) & (s_a <= 1) & (s_b >= 0) & (s_b <= 1)
            else:
                _, centre, radius = item
                oc = o - centre
                A, B, C = (d * d).sum(axis=1), 2.0 * (d @ oc), float(oc @ oc) - radius * radius
                disc = B * B - 4.0 * A * C
                t = (-B - np.sqrt(disc)) / (2.0 * A)
                ok = (disc >= 0) & (t > 0)
            best = np.where(ok & (t < best), t, best)
    xyz = np.where(np.isfinite(best)[:, None], best[:, None] * d_cam, np.nan)
    return xyz.astype(np.float32)


def corner_room(size=1.0):
    """Three mutually orthogonal square walls of edge ``size`` meeting at the origin of the world (the planes x = 0, y = 0, z = 0
    of the positive octant) and a sphere in front of the corner: every one of the six motions is held."""
    s = float(size)
    return [rectangle((0, 0, 0), (s, 0, 0), (0, s, 0)), rectangle((0, 0, 0), (0, s, 0), (0, 0, s)),
            rectangle((0, 0, 0), (0, 0, s), (s, 0, 0)), sphere((0.3 * s, 0.3 * s, 0.3 * s), 0.12 * s)]


def look_at(eye, at, up=(0.0, 0.0, 1.0)):
    """The camera-to-world pose of a camera at ``eye`` whose z axis points to ``at`` (x right, y down)."""
    eye, at, up = (np.asarray(v, dtype=np.float64) for v in (eye, at, up))
    z = at - eye
    z /= np.linalg.norm(z)
    x = np.cross(z, up)
    x /= np.linalg.norm(x)
    y = np.cross(z, x)
    T = np.eye(4)
    T[:3, 0], T[:3, 1], T[:3, 2], T[:3, 3] = x, y, z, eye
    return T
