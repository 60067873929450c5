"""Numpy restatement of the approach analysis against the TSDF volume (include/regnet_hip.h: regnet_grasp_approach_volume_f32;
regnet_for_3d_grasping_amd/approach_volume.py), written from the header's text and not from csrc/approach_volume.hip -- test
infrastructure, not product code.  float32 arrays, one operation per statement (numpy rounds each on its own and its division is
correctly rounded), every sample of the lattice visited for every grasp, nothing clipped and no tile or wave of the device
imitated: the contract reduces integer sums and float min / max only, so it has no order.

``approach_volume_ref`` is the kernel; ``derived_ref`` / ``passes_ref`` are ``VolumeApproach``'s tensors; the box and the
derivations shared with the cloud analysis are imported from ``approach_reference``.
"""
import math

import numpy as np

from . import approach_reference as cloud_ref

f32 = np.float32
INF = f32(np.inf)
MAX_SAMPLES = 1 << 22
gripper_box = cloud_ref.gripper_box


def lattice_counts(box, standoff, step, x_extent):
    """-> (n_x, n_y, n_z), xs, h: max(1, ceil(extent / h)) in float64 from the float32 constants."""
    x_lo, _, ht, hw, _, _ = box
    h = f32(float(step))
    xs = f32(f32(x_lo) - f32(standoff))
    extents = (float(f32(x_extent)) - float(xs), float(f32(hw)) + float(f32(hw)), float(f32(ht)) + float(f32(ht)))
    return tuple(max(1, int(math.ceil(e / float(h)))) for e in extents), xs, h


def lattice_samples(box, standoff, step, x_extent):
    """-> x (n_x), y (n_y), z (n_z) float32: the cell centres, never accumulated."""
    (n_x, n_y, n_z), xs, h = lattice_counts(box, standoff, step, x_extent)
    _, _, ht, hw, _, _ = box
    out = []
    for n, start in ((n_x, None), (n_y, f32(hw)), (n_z, f32(ht))):
        a = np.arange(n, dtype=np.float32) + f32(0.5)
        a = a * h
        out.append(xs + a if start is None else a - start)
    assert all(a.dtype == np.float32 for a in out)
    return out


def classify(vol_D, vol_W, dims, origin, voxel, min_weight, d_solid, L12, x, y, z):
    """One grasp's lookup of the samples (x, y, z broadcastable float32) -> inside, solid, unseen boolean arrays."""
    nx, ny, nz = dims
    l = np.asarray(L12, dtype=np.float32).reshape(3, 4)
    o = np.asarray(origin, dtype=np.float32)
    vx = f32(float(voxel))
    c = []
    with np.errstate(all="ignore"):
        for r in range(3):
            a = l[r, 0] * x
            b = l[r, 1] * y
            s = a + b
            b = l[r, 2] * z
            s = s + b
            w = s + l[r, 3]
            w = w - o[r]
            w = w / vx
            c.append(np.floor(w))
        assert all(a.dtype == np.float32 for a in c)
        inside = ((c[0] >= 0) & (c[0] < f32(nx)) & (c[1] >= 0) & (c[1] < f32(ny)) & (c[2] >= 0) & (c[2] < f32(nz)))
        ix, iy, iz = (np.where(inside, a, 0).astype(np.int64) for a in c)
        v = (iz * ny + iy) * nx + ix
        W = np.asarray(vol_W)[v]
        D = np.asarray(vol_D, dtype=np.float32)[v]
        known = inside & (W >= np.int32(min_weight)) & ~np.isnan(D)
        solid = known & (D < f32(d_solid))
    return inside, solid, ~known


def approach_volume_ref(vol_D, vol_W, dims, origin, voxel, trunc, min_weight, margin, L, box, standoff, step, x_extent):
    """-> counts (B,8) int32, values (B,4) float32.  ``L`` (B,12); ``box`` = (x_lo, x_hi scalar or (B), ht, hw, hs, back_x)."""
    x_lo, x_hi, ht, hw, hs, back_x = box
    x_lo, ht, hw, hs, back_x, S = f32(x_lo), f32(ht), f32(hw), f32(hs), f32(back_x), f32(standoff)
    L = np.asarray(L, dtype=np.float32).reshape(-1, 12)
    B = L.shape[0]
    xh_all = np.asarray(x_hi, dtype=np.float32).reshape(-1) if np.ndim(x_hi) else np.full((B,), x_hi, dtype=np.float32)
    d_solid = f32(float(margin) / float(trunc))
    (n_x, n_y, n_z), xs, _ = lattice_counts(box, standoff, step, x_extent)
    assert n_x * n_y * n_z <= MAX_SAMPLES
    xv, yv, zv = lattice_samples(box, standoff, step, x_extent)
    x, y, z = xv[:, None, None], yv[None, :, None], zv[None, None, :]
    shape = (n_x, n_y, n_z)
    counts = np.zeros((B, 8), dtype=np.int32)
    values = np.zeros((B, 4), dtype=np.float32)
    zero = f32(0.0)
    with np.errstate(all="ignore"):
        section = np.broadcast_to((z < ht) & (z > -ht) & (y < hw) & (y > -hw), shape)
        inner = section & (y < hs) & (y > -hs)
        retreat = np.broadcast_to(np.maximum(x_lo - x, zero), shape)
        yy = np.broadcast_to(y, shape)
        for b in range(B):
            xh = xh_all[b]
            close = (x > x_lo) & (x < xh)
            region = inner & close
            back = section & close & (x < back_x)
            finger = section & close & ((y > hs) | (y < -hs))
            front = np.where(inner, back_x, xh).astype(np.float32)
            blocker = section & (x < front) & (x > xs)
            hand = back.astype(np.int32) + finger.astype(np.int32)
            member = hand + blocker.astype(np.int32)
            looked = region | (member > 0)
            inside, solid, unseen = classify(vol_D, vol_W, dims, origin, voxel, min_weight, d_solid, L[b], x, y, z)
            solid, unseen, outside = solid & looked, unseen & looked, ~inside & looked
            counts[b] = [(region & solid).sum(), (region & unseen).sum(), hand[solid].sum(), hand[unseen].sum(),
                         (blocker & solid).sum(), (blocker & unseen).sum(), member[looked].sum(), member[outside].sum()]
            values[b, 0] = np.min(yy, initial=INF, where=region & solid) + zero
            values[b, 1] = np.max(yy, initial=-INF, where=region & solid) + zero
            values[b, 2] = np.minimum(S, np.min(retreat, initial=INF, where=blocker & solid)) + zero
            values[b, 3] = np.minimum(S, np.min(retreat, initial=INF, where=blocker & (solid | unseen))) + zero
    return counts, values


def derived_ref(counts, values, frame, center, pad, half_space, unseen="free", contact_counts=None):
    """``VolumeApproach``'s derived tensors -> dict of arrays, one float32 operation per step; ``contact_counts``: the (B,8)
    counts of the contact pass (``regnet_grasp_approach_f32`` on the surface) or None."""
    counts = np.asarray(counts, dtype=np.int32)
    values = np.asarray(values, dtype=np.float32)
    empty = counts[:, 0] == 0
    pad, hs = f32(pad), f32(half_space)
    with np.errstate(all="ignore"):
        width = np.where(empty, f32(0.0), values[:, 1] - values[:, 0]).astype(np.float32)
        offset = np.where(empty, f32(0.0), (values[:, 1] + values[:, 0]) * f32(0.5)).astype(np.float32)
        opening = np.minimum(width + f32(pad + pad), f32(hs + hs)).astype(np.float32)
        contact = np.zeros((len(counts),), dtype=np.float32)
        if contact_counts is not None:
            k = np.asarray(contact_counts, dtype=np.int32)
            c = k.astype(np.float32)
            share = (c[:, 4] / c[:, 3]) * (c[:, 6] / c[:, 5])
            contact = np.where((k[:, 3] == 0) | (k[:, 5] == 0), f32(0.0), share).astype(np.float32)
        clearance = values[:, 3 if unseen == "blocked" else 2].copy()
        approach = np.asarray(frame, dtype=np.float32)[:, :, 0]
        pregrasp = (np.asarray(center, dtype=np.float32) - approach * clearance[:, None]).astype(np.float32)
        share = (counts[:, 3] + counts[:, 5]).astype(np.float32) / counts[:, 6].astype(np.float32)
        unseen_share = np.where(counts[:, 6] == 0, f32(0.0), share).astype(np.float32)
    return {"grasp_clearance": clearance, "grasp_width": width, "grasp_offset": offset, "grasp_opening": opening,
            "grasp_contact": contact, "grasp_pregrasp": pregrasp, "grasp_clearance_seen": values[:, 2].copy(),
            "grasp_clearance_safe": values[:, 3].copy(), "grasp_unseen": unseen_share, "grasp_solid_hand": counts[:, 2].copy()}


passes_ref = cloud_ref.passes_ref


# ---- hand-built volumes ------------------------------------------------------------------------------------------------------
class HandVolume:
    """A volume set by hand: D = 1 / W = 0 (reset) unless written; ``at(ix, iy, iz)`` is a voxel's linear index."""

    def __init__(self, dims, origin, voxel, trunc=None, min_weight=1):
        self.dims = tuple(int(d) for d in dims)
        self.origin = np.asarray(origin, dtype=np.float64).astype(np.float32)
        self.voxel = float(voxel)
        self.trunc = 4.0 * self.voxel if trunc is None else float(trunc)
        self.min_weight = int(min_weight)
        n = self.dims[0] * self.dims[1] * self.dims[2]
        self.D = np.ones((n,), dtype=np.float32)
        self.W = np.zeros((n,), dtype=np.int32)

    def at(self, ix, iy, iz):
        nx, ny, nz = self.dims
        assert 0 <= ix < nx and 0 <= iy < ny and 0 <= iz < nz
        return (iz * ny + iy) * nx + ix

    def observe_all(self, d=1.0, w=1):
        self.D[:] = f32(d)
        self.W[:] = w
        return self

    def run(self, L, box, standoff, step, x_extent, margin=0.0):
        return approach_volume_ref(self.D, self.W, self.dims, self.origin, self.voxel, self.trunc, self.min_weight, margin, L, box,
                                   standoff, step, x_extent)


def rows_of(frame, center, to_volume=None):
    """L (B,12) float32 = to_volume @ [frame | centre] in float64, rounded once: what ``analyse_volume`` forms (tests that compare
    the kernel feed BOTH sides the rows the device computed; this one places hand-built cases)."""
    frame = np.asarray(frame, dtype=np.float64).reshape(-1, 3, 3)
    center = np.asarray(center, dtype=np.float64).reshape(-1, 3)
    M = np.zeros((len(frame), 4, 4))
    M[:, :3, :3], M[:, :3, 3], M[:, 3, 3] = frame, center, 1.0
    T = np.eye(4) if to_volume is None else np.asarray(to_volume, dtype=np.float64)
    return (T[None] @ M)[:, :3, :].reshape(-1, 12).astype(np.float32)
