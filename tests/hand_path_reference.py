"""Numpy restatement of the hand paths (include/regnet_hip.h "hand paths"; csrc/hand_path.hip, regnet_for_3d_grasping_amd/
hand_path.py), written from the header's text -- test infrastructure, not product code.  float32 arrays, one operation per
statement; every hand sample at every waypoint of every path, nothing clipped; a plain ``min``; the prefix rule as a plain loop.
The lookup (``affine3`` and ``grid_voxel``) is ``edt_reference.lookup``, the lattice ``approach_volume_reference``'s and the hand's
sets ``retreat_reference.hand_samples``, imported; the pick is ``retreat_reference.pick_ref`` (the kernel is the fan's).  No tile,
wave or LDS word of the device is imitated.
"""
import math

import numpy as np

from . import edt_reference as edt_ref
from . import retreat_reference as fan_ref
from . import sdf_reference as sdf_ref

f32 = np.float32
NONE = edt_ref.NONE
pick_ref = fan_ref.pick_ref


def _x_hi_all(box, B):
    x_hi = box[1]
    return np.asarray(x_hi, dtype=np.float32).reshape(-1) if np.ndim(x_hi) else np.full((B,), x_hi, dtype=np.float32)


def path_ref(field, dims, origin, voxel, outside, P, box, step, x_extent, thresh, signed):
    """``P`` (B,R,K+1,12) -> profile (B,R,K+1) int32, result (B,R,4) int32.  ``box`` = (x_lo, x_hi scalar or (B), ht, hw, hs,
    back_x)."""
    P = np.asarray(P, dtype=np.float32)
    B, R, K1, _ = P.shape
    K = K1 - 1
    xh_all = _x_hi_all(box, B)
    words = np.asarray(field, dtype=np.int64)
    profile = np.full((B, R, K + 1), NONE, dtype=np.int32)
    result = np.zeros((B, R, 4), dtype=np.int32)
    for b in range(B):
        x, y, z, hand = fan_ref.hand_samples(box, step, x_extent, xh_all[b])
        points = np.stack([x[hand], y[hand], z[hand]], axis=1)
        for r in range(R):
            n_out = 0
            for k in range(K + 1):
                inside, v = edt_ref.lookup(points, P[b, r, k], dims, origin, voxel)
                value = np.where(inside, words[v], -1 if signed else 0)
                counted = inside | bool(outside)
                profile[b, r, k] = min([NONE] + value[counted].tolist())
                if k > 0:
                    n_out += int((~inside).sum())
            free_steps = 0
            for k in range(1, K + 1):
                if profile[b, r, k] >= thresh:
                    free_steps = k
                else:
                    break
            free_min = min([NONE] + profile[b, r, 1:free_steps + 1].tolist())
            all_min = min([NONE] + profile[b, r, 1:].tolist())
            result[b, r] = [free_steps, free_min, all_min, n_out]
    return profile, result


def _apply(rows, c):
    """affine3 of the three rows (12 float32) to the float32 point ``c`` -> three float32."""
    t = np.asarray(rows, dtype=np.float32).reshape(3, 4)
    out = []
    for i in range(3):
        a = t[i, 0] * c[0]
        b = t[i, 1] * c[1]
        s = a + b
        b = t[i, 2] * c[2]
        s = s + b
        out.append(s + t[i, 3])
    return out


def disp_ref(P, box):
    """-> (B,R,K) float32: per step the largest distance a corner of the hand's bounding box moves, NaN when any is one."""
    P = np.asarray(P, dtype=np.float32)
    B, R, K1, _ = P.shape
    xh_all = _x_hi_all(box, B)
    x_lo, _, ht, hw, _, _ = box
    out = np.zeros((B, R, K1 - 1), dtype=np.float32)
    with np.errstate(all="ignore"):
        for b in range(B):
            corners = [(f32(cx), f32(cy), f32(cz)) for cx in (f32(x_lo), xh_all[b]) for cy in (-f32(hw), f32(hw))
                       for cz in (-f32(ht), f32(ht))]
            for r in range(R):
                for k in range(K1 - 1):
                    far = f32(0.0)
                    for c in corners:
                        p0 = _apply(P[b, r, k], c)
                        p1 = _apply(P[b, r, k + 1], c)
                        dx = p1[0] - p0[0]
                        dy = p1[1] - p0[1]
                        dz = p1[2] - p0[2]
                        xx = dx * dx
                        yy = dy * dy
                        zz = dz * dz
                        s = xx + yy
                        s = s + zz
                        root = np.sqrt(s)
                        assert root.dtype == np.float32
                        far = np.maximum(far, root)          # (np.maximum hands a NaN on)
                    out[b, r, k] = far
    return out


def compose_ref(L, local):
    """``L`` (B,12) float32, ``local`` (R,K+1,12) or (B,R,K+1,12) float32 -> P (B,R,K+1,12) float32: float64 products summed in
    the stated order, rounded once."""
    L = np.asarray(L, dtype=np.float32).reshape(-1, 3, 4).astype(np.float64)
    local = np.asarray(local, dtype=np.float32).astype(np.float64)
    B = L.shape[0]
    local = np.broadcast_to(local, (B,) + local.shape[-3:]) if local.ndim == 3 else local
    R, K1 = local.shape[1], local.shape[2]
    m = local.reshape(B, R, K1, 3, 4)
    out = np.zeros((B, R, K1, 3, 4), dtype=np.float64)
    for i in range(3):
        for j in range(4):
            a = L[:, i, 0, None, None] * m[:, :, :, 0, j]
            b = L[:, i, 1, None, None] * m[:, :, :, 1, j]
            s = a + b
            b = L[:, i, 2, None, None] * m[:, :, :, 2, j]
            s = s + b
            if j == 3:
                s = s + L[:, i, 3, None, None]
            out[:, :, :, i, j] = s
    return out.reshape(B, R, K1, 12).astype(np.float32)


def metres_ref(profile, voxel, signed):
    profile = np.asarray(profile, dtype=np.int32)
    flat = profile.reshape(-1)
    out = sdf_ref.metres_signed_ref(flat, voxel) if signed else edt_ref.metres_ref(flat, voxel)
    return np.asarray(out, dtype=np.float32).reshape(profile.shape)


def default_slack(step, voxel):
    return (float(step) + float(voxel)) * math.sqrt(3.0) / 2.0


def certified_ref(profile, disp, voxel, signed, slack, min_margin):
    """-> (B,R) int32: the prefix of steps k with ((min(m[k-1], m[k]) - disp[k-1] / 2) - slack) >= min_margin in float32."""
    metres = metres_ref(profile, voxel, signed)
    disp = np.asarray(disp, dtype=np.float32)
    B, R, K = disp.shape
    out = np.zeros((B, R), dtype=np.int32)
    with np.errstate(all="ignore"):
        for b in range(B):
            for r in range(R):
                for k in range(1, K + 1):
                    low = np.minimum(metres[b, r, k - 1], metres[b, r, k])
                    half = disp[b, r, k - 1] / f32(2.0)
                    room = low - half
                    room = room - f32(slack)
                    assert room.dtype == np.float32
                    if not room >= f32(min_margin):
                        break
                    out[b, r] = k
    return out


def waypoint_ref(P, best):
    """-> (B,12): the picked path's pose at its last free step."""
    P = np.asarray(P, dtype=np.float32)
    return np.stack([P[b, best[b, 0], best[b, 1]] for b in range(P.shape[0])])


def length_ref(disp, best, steps):
    """-> (B) float32: the picked path's ``disp`` summed in float32 from the left over its first ``steps[b]`` entries."""
    disp = np.asarray(disp, dtype=np.float32)
    out = np.zeros((disp.shape[0],), dtype=np.float32)
    for b in range(disp.shape[0]):
        total = f32(0.0)
        for k in range(int(steps[b])):
            total = total + disp[b, best[b, 0], k]
        assert total.dtype == np.float32
        out[b] = total
    return out
