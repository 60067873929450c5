"""numpy restatement of the raycast of the TSDF volume and of the frame-to-model tracking loop around it (include/regnet_hip.h,
DESIGN.md par. 5 "Raycast and tracking"), written from the contract text and not from csrc/tsdf.hip: float32 arrays, one
operation per statement (numpy rounds each on its own; its division and square root are correctly rounded), a Python loop over
the samples of ALL rays at once.  Nothing is clipped: every ray visits every sample, which is what makes the comparison with
the device a test of its clip.  The volume is ``tsdf_reference.Volume``; the renderer and the registration are
``icp_projective_reference``'s, imported and not copied.
"""
import math

import numpy as np

from .icp_projective_reference import DEGENERATE, TOO_FEW, icp_projective, look_at, rectangle, render, sphere  # noqa: F401
from .tsdf_reference import Volume, constants  # noqa: F401

f32 = np.float32
NO_SURFACE, BACK_FACE, HIT, HIT_NO_NORMAL = 0, 1, 2, 3
FIRST, TRACKED, LOST = "FIRST", "TRACKED", "LOST"
QNAN = np.array([0x7FC00000], dtype=np.uint32).view(np.float32)[0]
TRACK_DEFAULTS = dict(max_dist=0.02, iterations=20, stride=1, window=1, min_pairs=100, rot_eps=1e-5, trans_eps=1e-6, min_cos=None,
                      near=0.2, far=1.5, step=None, max_translation=0.05, max_rotation=0.1, min_hit_share=0.05)


def intrinsics4(intrinsics):
    """(fx, fy, cx, cy) -> rfx = float32(1 / fx), rfy, cx, cy: the reciprocals in float64, rounded once."""
    fx, fy, cx, cy = (float(v) for v in intrinsics)
    return f32(1.0 / fx), f32(1.0 / fy), f32(cx), f32(cy)


def pose_rows(pose):
    """Rows 0..2 of the camera-to-common 4x4 (None: identity) as 12 float32, rounded once, not inverted."""
    T = np.eye(4) if pose is None else np.asarray(pose, dtype=np.float64)
    return T[:3, :].reshape(12).astype(np.float32)


def steps(near, far, step):
    """n_steps = ceil((far - near) / step), in float64."""
    return int(math.ceil((float(far) - float(near)) / float(step)))


def camera_point(du, dv, z, k4):
    """c = ((du * z) * rfx, (dv * z) * rfy, z) for arrays du, dv and z (an array or one float32) -> (m,3) float32."""
    a = du * z
    x = a * k4[0]
    b = dv * z
    y = b * k4[1]
    c = np.stack([x, y, np.broadcast_to(z, x.shape).astype(np.float32)], axis=1)
    assert c.dtype == np.float32
    return c


def common_point(c, r):
    """p_k = (((r_k0 c_x) + (r_k1 c_y)) + (r_k2 c_z)) + t_k -> (m,3) float32."""
    out = []
    for k in range(3):
        a = r[4 * k] * c[:, 0]
        b = r[4 * k + 1] * c[:, 1]
        d = r[4 * k + 2] * c[:, 2]
        s = a + b
        s = s + d
        out.append(s + r[4 * k + 3])
    p = np.stack(out, axis=1)
    assert p.dtype == np.float32
    return p


def cell(vol, p):
    """-> (inside (m,), l (m,) int64: the lower corner's linear index, 0 where not inside, f (m,3) float32)."""
    nx, ny, _ = vol.dims
    inside = np.ones((len(p),), dtype=bool)
    lower, frac = [], []
    for k in range(3):
        d = p[:, k] - vol.origin[k]
        q = d / vol.voxel
        g = q - f32(0.5)
        fl = np.floor(g)
        fr = g - fl
        up = fl + f32(1.0)
        assert fl.dtype == fr.dtype == up.dtype == np.float32
        inside &= (fl >= f32(0.0)) & (up <= f32(vol.dims[k] - 1))
        lower.append(fl)
        frac.append(fr)
    i = [np.where(inside, fl, f32(0.0)).astype(np.int64) for fl in lower]
    return inside, (i[2] * ny + i[1]) * nx + i[0], np.stack(frac, axis=1)


def corners(vol, l):
    """The eight linear indices of the cell at ``l``, x fastest: (m,8) in the order 000, 100, 010, 110, 001, 101, 011, 111."""
    nx, ny, _ = vol.dims
    return np.stack([l + a + b * nx + c * nx * ny for c in (0, 1) for b in (0, 1) for a in (0, 1)], axis=1)


def trilinear(values, f):
    """``values`` (m,8) in ``corners``' order: a + (f * (b - a)) along x, then y, then z -> (m,) float32."""
    def mix(a, b, t):
        d = b - a
        d = t * d
        return a + d
    c00, c10 = mix(values[:, 0], values[:, 1], f[:, 0]), mix(values[:, 2], values[:, 3], f[:, 0])
    c01, c11 = mix(values[:, 4], values[:, 5], f[:, 0]), mix(values[:, 6], values[:, 7], f[:, 0])
    c0, c1 = mix(c00, c10, f[:, 1]), mix(c01, c11, f[:, 1])
    out = mix(c0, c1, f[:, 2])
    assert out.dtype == np.float32
    return out


def sample(vol, p, plane=None):
    """S(p) for ``p`` (m,3) float32 -> (known (m,), value (m,) float32, anything where unknown).  ``plane``: (N,) float32 to
    interpolate instead of D."""
    inside, l, f = cell(vol, p)
    c = corners(vol, l)
    known = inside & (vol.W[c].min(axis=1) >= np.int32(vol.p["min_weight"]))
    return known, trilinear((vol.D if plane is None else plane)[c], f)


def raycast(vol, pose, intrinsics, width, height, near, step, n_steps, colour=True):
    """The model view -> dict: ``xyz``, ``normals`` (H W, 3) float32 in the virtual camera's frame, ``rgb`` (H W, 3) float32 or
    None, ``status`` (H W) uint8, ``counts`` (4) int32, and ``z`` (H W) float32, the depth of the hit (NaN without one)."""
    W, H = int(width), int(height)
    k4 = intrinsics4(intrinsics)
    r = pose_rows(pose)
    near, step = f32(float(near)), f32(float(step))
    v, u = np.divmod(np.arange(W * H, dtype=np.int64), W)
    du = u.astype(np.float32) - k4[2]
    dv = v.astype(np.float32) - k4[3]
    status = np.full((W * H,), NO_SURFACE, dtype=np.uint8)
    previous = np.zeros((W * H,), dtype=bool)                  # the last sample was known with a value > 0
    v_prev = np.zeros((W * H,), dtype=np.float32)
    z_prev = np.zeros((W * H,), dtype=np.float32)
    z_hit = np.full((W * H,), np.nan, dtype=np.float32)
    alive = np.ones((W * H,), dtype=bool)
    with np.errstate(all="ignore"):
        for i in range(int(n_steps)):
            rows = np.nonzero(alive)[0]
            if len(rows) == 0:
                break
            z = f32(i) * step
            z = near + z
            assert z.dtype == np.float32
            p = common_point(camera_point(du[rows], dv[rows], z, k4), r)
            known, value = sample(vol, p)
            below = known & (value <= f32(0.0))
            hit = below & previous[rows]
            den = v_prev[rows] - value
            s = v_prev[rows] / den
            zh = s * step
            zh = z_prev[rows] + zh
            z_hit[rows[hit]] = zh[hit]
            status[rows[hit]] = HIT_NO_NORMAL
            status[rows[below & ~previous[rows]]] = BACK_FACE
            alive[rows[below]] = False
            previous[rows] = known & (value > f32(0.0))
            v_prev[rows] = value
            z_prev[rows] = z
        xyz = np.full((W * H, 3), QNAN, dtype=np.float32)
        normals = np.full((W * H, 3), QNAN, dtype=np.float32)
        rgb = np.zeros((W * H, 3), dtype=np.float32) if colour else None
        rows = np.nonzero(status == HIT_NO_NORMAL)[0]
        c = camera_point(du[rows], dv[rows], z_hit[rows], k4)
        p = common_point(c, r)
        xyz[rows] = c
        if colour:
            for k in range(3):
                known, value = sample(vol, p, vol.C[:, k])
                rgb[rows, k] = np.where(known, value, f32(0.0))
        g, all_known = [], np.ones((len(rows),), dtype=bool)
        for k in range(3):
            q = p.copy()
            q[:, k] = p[:, k] + vol.voxel
            known_hi, hi = sample(vol, q)
            q = p.copy()
            q[:, k] = p[:, k] - vol.voxel
            known_lo, lo = sample(vol, q)
            all_known &= known_hi & known_lo
            g.append(hi - lo)
        n = []
        for k in range(3):                                     # the transpose of the rotation
            a = r[k] * g[0]
            b = r[4 + k] * g[1]
            d = r[8 + k] * g[2]
            s = a + b
            n.append(s + d)
        len2 = n[0] * n[0]
        len2 = len2 + (n[1] * n[1])
        len2 = len2 + (n[2] * n[2])
        ok = all_known & np.isfinite(len2) & (len2 > f32(0.0))
        length = np.sqrt(len2)
        n = [t / length for t in n]
        dot = n[0] * c[:, 0]
        dot = dot + (n[1] * c[:, 1])
        dot = dot + (n[2] * c[:, 2])
        flip = dot > f32(0.0)
        n = np.stack([np.where(flip, -t, t) for t in n], axis=1)
        assert n.dtype == len2.dtype == np.float32
        normals[rows[ok]] = n[ok]
        status[rows[ok]] = HIT
    return {"xyz": xyz, "normals": normals, "rgb": rgb, "status": status, "z": z_hit,
            "counts": np.bincount(status, minlength=4).astype(np.int32)}


def relative_motion(T):
    """A rigid 4x4 -> (the length of its translation, its rotation angle [rad])."""
    T = np.asarray(T, dtype=np.float64)
    cos = min(1.0, max(-1.0, (float(np.trace(T[:3, :3])) - 1.0) / 2.0))
    return float(np.linalg.norm(T[:3, 3])), math.acos(cos)


def track(frames, width, height, intrinsics, volume_params, track_params=None, first_pose=None, guesses=None, source_normals=None):
    """The whole loop.  ``frames``: per frame ``(xyz, rgb)``, the organised cloud in its camera's frame (rgb may be None);
    ``guesses``: per frame a pose to raycast from instead of the last one, or None; ``source_normals``: per frame the normals the
    gate ``min_cos`` compares, or None -> (Volume, [dict(pose, status, report, counts, model)]): the first frame is integrated at
    ``first_pose`` (identity); every later one is registered onto the raycast from the last pose and integrated at the pose
    found, or LOST: nothing is integrated and the pose is kept."""
    t = dict(TRACK_DEFAULTS)
    t.update(track_params or {})
    vol = Volume(**volume_params)
    step = float(vol.p["trunc"]) / 2.0 if t["step"] is None else float(t["step"])
    n = steps(t["near"], t["far"], step)
    icp_params = {k: t[k] for k in ("max_dist", "iterations", "stride", "window", "min_pairs", "rot_eps", "trans_eps", "min_cos")}
    pose = np.eye(4) if first_pose is None else np.array(first_pose, dtype=np.float64)
    out = []
    for j, (xyz, rgb) in enumerate(frames):
        if j == 0:
            counts = vol.integrate(xyz, rgb, width, height, intrinsics, pose)
            out.append({"pose": pose.copy(), "status": FIRST, "report": None, "counts": counts, "model": None})
            continue
        at = pose if guesses is None or guesses[j] is None else np.asarray(guesses[j], dtype=np.float64)
        model = raycast(vol, at, intrinsics, width, height, t["near"], step, n, colour=False)
        reg = icp_projective(xyz, model["xyz"], model["normals"], width, height, intrinsics, None, icp_params,
                             None if source_normals is None else source_normals[j])
        hits = int(model["counts"][HIT]) + int(model["counts"][HIT_NO_NORMAL])
        moved, turned = relative_motion(reg["pose"])
        lost = (reg["status"] in (TOO_FEW, DEGENERATE) or hits < t["min_hit_share"] * width * height
                or moved > t["max_translation"] or turned > t["max_rotation"])
        if lost:
            out.append({"pose": pose.copy(), "status": LOST, "report": reg, "counts": None, "model": model})
            continue
        pose = at @ reg["pose"]
        counts = vol.integrate(xyz, rgb, width, height, intrinsics, pose)
        out.append({"pose": pose.copy(), "status": TRACKED, "report": reg, "counts": counts, "model": model})
    return vol, out
