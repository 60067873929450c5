"""Numpy restatement of the retreat fan (include/regnet_hip.h "retreat fan"; csrc/retreat.hip, regnet_for_3d_grasping_amd/
retreat.py), written from the header's text -- test infrastructure, not product code.  float32 arrays, one operation per
statement; every lattice sample at every step of every direction, nothing skipped; a plain ``min``; the prefix rule and the pick as
plain loops.  The lookup is ``edt_reference.lookup`` and the lattice ``approach_volume_reference``'s, imported; the hand's sets are
written as ``edt_reference.margin_ref`` writes them (neither reference exports them as a function).  No tile, wave or LDS word of
the device is imitated: the contract reduces integer minima and sums only, so it has no order.
"""
import numpy as np

from . import approach_volume_reference as av_ref
from . import edt_reference as edt_ref

f32 = np.float32
NONE = edt_ref.NONE


def hand_samples(box, step, x_extent, xh):
    """The lattice of the hand at its final pose (standoff 0) -> x, y, z (n) float32 of ALL samples and hand (n) bool: back ||
    finger for the grasp's own ``xh``, a sample that is both counted once."""
    x_lo, _, ht, hw, hs, back_x = box
    x_lo, ht, hw, hs, back_x, xh = f32(x_lo), f32(ht), f32(hw), f32(hs), f32(back_x), f32(xh)
    xv, yv, zv = av_ref.lattice_samples(box, 0.0, step, x_extent)
    x, y, z = np.meshgrid(xv, yv, zv, indexing="ij")
    x, y, z = x.reshape(-1), y.reshape(-1), z.reshape(-1)
    with np.errstate(all="ignore"):
        section = (z < ht) & (z > -ht) & (y < hw) & (y > -hw)
        close = (x > x_lo) & (x < xh)
        back = section & close & (x < back_x)
        finger = section & close & ((y > hs) | (y < -hs))
    return x, y, z, back | finger


def fan_ref(field, dims, origin, voxel, outside, L, box, step, x_extent, dirs, K, ds, thresh, signed):
    """-> profile (B,R,K+1) int32, result (B,R,4) int32.  ``dirs`` (R,3) shared or (B,R,3); ``box`` = (x_lo, x_hi scalar or (B),
    ht, hw, hs, back_x)."""
    L = np.asarray(L, dtype=np.float32).reshape(-1, 12)
    B = L.shape[0]
    dirs = np.asarray(dirs, dtype=np.float32)
    dirs = np.broadcast_to(dirs, (B,) + dirs.shape[-2:]) if dirs.ndim == 2 else dirs
    R = dirs.shape[1]
    x_hi = box[1]
    xh_all = np.asarray(x_hi, dtype=np.float32).reshape(-1) if np.ndim(x_hi) else np.full((B,), x_hi, dtype=np.float32)
    words = np.asarray(field, dtype=np.int64)
    ds_f = f32(float(ds))
    profile = np.full((B, R, K + 1), NONE, dtype=np.int32)
    result = np.zeros((B, R, 4), dtype=np.int32)
    for b in range(B):
        x, y, z, hand = hand_samples(box, step, x_extent, xh_all[b])
        x, y, z = x[hand], y[hand], z[hand]
        for r in range(R):
            d = dirs[b, r]
            n_out = 0
            for k in range(K + 1):
                with np.errstate(all="ignore"):
                    t = f32(k) * ds_f
                    ax = t * d[0]
                    ay = t * d[1]
                    az = t * d[2]
                    px = x + ax
                    py = y + ay
                    pz = z + az
                assert px.dtype == np.float32 and t.dtype == np.float32
                inside, v = edt_ref.lookup(np.stack([px, py, pz], axis=1), L[b], dims, origin, voxel)
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


def pick_ref(result):
    """(B,R,4) -> best (B,4) int32: most free steps, then the larger free-prefix minimum, then the smaller r."""
    result = np.asarray(result, dtype=np.int32)
    best = np.zeros((result.shape[0], 4), dtype=np.int32)
    for b in range(result.shape[0]):
        pick = 0
        for r in range(1, result.shape[1]):
            steps, margin = int(result[b, r, 0]), int(result[b, r, 1])
            if steps > result[b, pick, 0]:
                pick = r
            elif steps == result[b, pick, 0] and margin > result[b, pick, 1]:
                pick = r
        best[b] = [pick, result[b, pick, 0], result[b, pick, 1], 0]
    return best


def threshold_ref(min_margin, voxel, signed):
    """The smallest field word whose metres value is >= float32(min_margin), by a scan of the words in ascending order over a
    window that holds the answer: the words up to ``(ceil(|min_margin| / voxel) + 2)^2`` either side (a root grows by less than
    a unit per unit of distance); NONE when the bound is beyond every finite word of a 1024^3 field."""
    from . import sdf_reference as sdf_ref
    bound = f32(min_margin)
    reach = int(np.ceil(abs(float(min_margin)) / float(voxel))) + 2
    top = min(reach * reach, 3 * 1023 * 1023)
    if signed:
        words = np.array([-NONE] + [w for w in range(-top, top + 1) if w != 0] + [NONE], dtype=np.int64)
        metres = sdf_ref.metres_signed_ref(words.astype(np.int32), voxel)
    else:
        words = np.array(list(range(0, top + 1)) + [NONE], dtype=np.int64)
        metres = edt_ref.metres_ref(words.astype(np.int32), voxel)
    return int(words[np.flatnonzero(metres >= bound)[0]])
