"""Numpy restatement of the push-out (include/regnet_hip.h "push-out"; csrc/hand_adjust.hip, regnet_for_3d_grasping_amd/
hand_adjust.py), written from the header's text -- test infrastructure, not product code.  float32 scalars and arrays, one
operation per statement; every hand sample at every iterate, nothing clipped; the minimum is a plain ``min`` over the 64-bit keys
the header defines; the iteration and its decisions are a plain loop.  The interpolated value and its gradient are
``sdf_reference.query_signed_ref`` (which also applies the rows and decides INSIDE) and the hand's samples
``retreat_reference.hand_samples``, imported.  No tile, wave or LDS word of the device is imitated.
"""
import numpy as np

from . import retreat_reference as fan_ref
from . import sdf_reference as sdf_ref

f32 = np.float32
ALREADY_FREE, FREED, MAX_ITER, CAPPED, STUCK, LEFT_VOLUME = range(6)
NAMES = ("ALREADY_FREE", "FREED", "MAX_ITER", "CAPPED", "STUCK", "LEFT_VOLUME")
QNAN = sdf_ref.QNAN


def ordered(values):
    """float32 -> uint32: ``b ^ ((b >> 31) | 0x80000000)`` of the bits as int32, the shift arithmetic."""
    b = np.asarray(values, dtype=np.float32).view(np.int32)
    return (b ^ ((b >> 31) | np.int32(-(1 << 31)))).view(np.uint32)


def _dot3(ax, ay, az, bx, by, bz):
    xx = ax * bx
    yy = ay * by
    zz = az * bz
    s = xx + yy
    return s + zz


def _x_hi_all(box, B):
    x_hi = box[1]
    return np.asarray(x_hi, dtype=np.float32).reshape(-1) if np.ndim(x_hi) else np.full((B,), x_hi, dtype=np.float32)


def push_out_ref(field, dims, origin, voxel, outside, L, box, step, x_extent, axes, target, max_shift, T):
    """-> pose (B,12) float32, shift (B,3) float32, trace (B,T+1) float32, info (B,4) int32.  ``box`` = (x_lo, x_hi scalar or
    (B), ht, hw, hs, back_x)."""
    L = np.asarray(L, dtype=np.float32).reshape(-1, 12)
    B = L.shape[0]
    xh_all = _x_hi_all(box, B)
    axes = np.asarray(axes, dtype=np.float32).reshape(3)
    target_f = f32(float(target))
    cap_f = f32(float(max_shift))
    pose = L.copy()
    shift = np.zeros((B, 3), dtype=np.float32)
    trace = np.full((B, T + 1), QNAN, dtype=np.float32)
    info = np.zeros((B, 4), dtype=np.int32)
    with np.errstate(all="ignore"):
        cap2 = cap_f * cap_f
        for b in range(B):
            x, y, z, hand = fan_ref.hand_samples(box, step, x_extent, xh_all[b])
            index = np.flatnonzero(hand)
            points = np.stack([x[index], y[index], z[index]], axis=1)
            rows = L[b].copy()
            t0 = [rows[3], rows[7], rows[11]]
            s = [f32(0.0), f32(0.0), f32(0.0)]
            steps, n = 0, 0
            while True:
                if len(index):
                    value, gradient, _ = sdf_ref.query_signed_ref(field, None, dims, origin, voxel, points, T12=rows, interpolate=True)
                else:
                    value, gradient = np.zeros((0,), dtype=np.float32), np.zeros((0, 3), dtype=np.float32)
                valued = ~np.isnan(value)                # OUTSIDE is a NaN here, and a NaN value counts as OUTSIDE
                n_out = int((~valued).sum())
                worst, low = -1, f32(np.inf)
                if valued.any():
                    keys = (ordered(value[valued]).astype(np.uint64) << np.uint64(32)) | index[valued].astype(np.uint64)
                    at = np.flatnonzero(valued)[int(np.argmin(keys))]
                    assert keys.min() == (np.uint64(ordered(value[at:at + 1])[0]) << np.uint64(32)) | np.uint64(index[at])
                    worst, low = int(index[at]), value[at]
                trace[b, n] = low
                info[b, 2:] = [worst, n_out]
                if worst < 0 and n_out == 0:
                    status = ALREADY_FREE
                    break
                if worst < 0 or (outside and n_out > 0):
                    status = LEFT_VOLUME
                    break
                if low >= target_f:
                    status = ALREADY_FREE if n == 0 else FREED
                    break
                if n == T:
                    status = MAX_ITER
                    break
                g = gradient[at]
                a = [axes[k] * _dot3(rows[k], rows[4 + k], rows[8 + k], g[0], g[1], g[2]) for k in range(3)]
                e = target_f - low
                d = [e * a[k] for k in range(3)]
                assert all(v.dtype == np.float32 for v in a + d) and e.dtype == np.float32
                if any(np.isnan(v) for v in a) or all(v == 0 for v in d):
                    status = STUCK
                    break
                c = [s[k] + d[k] for k in range(3)]
                if not _dot3(c[0], c[1], c[2], c[0], c[1], c[2]) <= cap2:
                    status = CAPPED
                    break
                s = c
                steps += 1
                n += 1
                for i in range(3):
                    rows[4 * i + 3] = _dot3(rows[4 * i], rows[4 * i + 1], rows[4 * i + 2], s[0], s[1], s[2]) + t0[i]
            pose[b] = rows
            shift[b] = s
            info[b, :2] = [status, steps]
    return pose, shift, trace, info
