"""Outlier removal on the device (csrc/outlier.hip): the radius filter of the reference's ``PointCloud.remove_outliers``
(dataset_utils/eval_score/eval_utils/pointcloud.py: open3d's ``remove_radius_outlier``) and open3d / PCL's statistical outlier
removal, over the rows of a cloud that a mask keeps and whose coordinates are finite (the graph rows).

``radius_count`` gives every graph row the number of OTHER graph rows within ``radius``, saturated at ``min_neighbours``; a row
is an inlier when it reaches it.  ``knn_mean_distance`` gives it the mean distance to its ``k`` nearest neighbours within
``max_radius``; the statistical filter keeps the rows whose mean is at most ``mu + std_ratio * sigma`` of the cloud's means.
``filter_cloud`` runs one of them or the first and then the second on its survivors, and ``Filtered.apply`` blanks the removed
rows (NaN coordinates, rgb 0), which every later stage treats as absent.  The arithmetic is pinned (include/regnet_hip.h,
DESIGN.md par. 5): float32 distances, every operation rounded on its own, float64 sums in a fixed order, so
``tests/outlier_reference.py`` restates it in numpy and the two agree bit for bit.

Nothing here reads from the device except ``Filtered.counts()``; nothing draws from numpy's random stream.  GPU only: there is no
CPU path.
"""
from dataclasses import dataclass

import numpy as np
import torch

from . import _lib
from ._frame_util import ParamsBase, require_cuda

_L = _lib.lib

MODES = ("radius", "statistical", "both")
# Filtered.status, the first that applies
NOT_A_ROW, TOO_FEW_IN_RADIUS, TOO_FEW_NEAREST, TOO_FAR, KEPT = 0, 1, 2, 3, 4
MAX_KNN = 64


@dataclass
class OutlierParams(ParamsBase):
    """What ``GraspDetector(denoise=...)`` takes (a dict with these keys works too).  ``mode``: ``"radius"``, ``"statistical"``
    or ``"both"`` (the radius filter, then the statistical one on its survivors).  ``radius`` [m] / ``min_neighbours``: a row
    stays when at least so many other rows lie within the radius.  ``knn`` / ``max_radius`` [m]: the mean distance to the so many
    nearest rows within that radius; a row with fewer is removed.  ``std_ratio``: a row stays when its mean distance is at most
    the cloud's mean plus so many standard deviations.

    ``radius`` and ``min_neighbours`` are the reference's ``RADIUS_THRESHOLD`` and ``NUM_POINTS_THRESHOLD``
    (eval_score/configs/config.py); the others are a choice.  Nobody has measured any of the defaults on real frames."""
    WORD = "denoise"
    mode: str = "radius"
    radius: float = 0.04
    min_neighbours: int = 16
    knn: int = 20
    max_radius: float = 0.04
    std_ratio: float = 2.0

    def __post_init__(self):
        if self.mode not in MODES:
            raise ValueError("denoise: mode must be one of %s, not %r" % (", ".join(MODES), self.mode))
        for name in ("radius", "max_radius"):
            with np.errstate(over="ignore"):
                value = np.float32(getattr(self, name))
            if not (value > 0.0 and np.isfinite(value)):
                raise ValueError("denoise: %s must be positive and finite in float32" % name)
        if int(self.min_neighbours) < 1:
            raise ValueError("denoise: min_neighbours must be at least 1")
        if not 1 <= int(self.knn) <= MAX_KNN:
            raise ValueError("denoise: knn must be between 1 and %d" % MAX_KNN)
        if not (float(self.std_ratio) >= 0.0 and np.isfinite(self.std_ratio)):
            raise ValueError("denoise: std_ratio must be non-negative and finite")


class Filtered:
    """``filter_cloud``'s result, all on the device: ``keep`` (N) bool; ``status`` (N) uint8 = 0 not a graph row, 1 too few rows
    within ``radius``, 2 fewer than ``knn`` rows within ``max_radius``, 3 mean distance above the threshold, 4 kept (the first
    that applies); ``num`` (5) int32, the histogram of ``status``; ``stats`` (4) float64 = (n, mu, sigma, threshold) of the
    statistical stage and ``mean_dist`` (N) float32, both None in mode ``"radius"``; ``count`` (N) int32 of the radius stage, None
    in mode ``"statistical"``; ``found`` (N) int32 beside ``mean_dist``."""

    def __init__(self, keep, status, num, stats=None, mean_dist=None, count=None, found=None):
        self.keep, self.status, self.num, self.stats = keep, status, num, stats
        self.mean_dist, self.count, self.found = mean_dist, count, found

    def apply(self, xyz, rgb=None):
        """Copies of ``xyz`` (N,3) (and ``rgb``) with the removed rows set to the quiet NaN (rgb: 0): dtype and row organisation
        are kept, the caller's tensors are untouched.  -> ``xyz`` or ``(xyz, rgb)``."""
        _cuda("xyz", xyz, (torch.float32, torch.float64), 3)
        if xyz.shape[0] != self.keep.shape[0]:
            raise RuntimeError("apply: xyz must have the rows of the filtered cloud")
        keep = self.keep[:, None]
        out = torch.where(keep, xyz, torch.full((), float("nan"), dtype=xyz.dtype, device=xyz.device))
        if rgb is None:
            return out
        if not isinstance(rgb, torch.Tensor) or rgb.device != xyz.device or rgb.dim() != 2 or rgb.shape[0] != xyz.shape[0]:
            raise RuntimeError("apply: rgb must be a tensor on xyz's device with one row per row of xyz")
        return out, torch.where(keep, rgb, torch.zeros((), dtype=rgb.dtype, device=rgb.device))

    def counts(self):
        """The one blocking read: ``num`` -> a tuple of five ints (status 0..4)."""
        return tuple(int(v) for v in self.num.cpu())


def workspace_bytes(n):
    """Bytes of scratch the two searches need for ``n`` rows."""
    return int(_L.regnet_outlier_workspace_bytes(int(n)))


def _cuda(name, x, dtype=None, cols=None):
    """Every argument check of this module is a RuntimeError."""
    return require_cuda(name, x, dtype, cols, error=RuntimeError)


def _inputs(xyz, mask):
    """-> (xyz as contiguous float32, mask as contiguous uint8 or None, the mask's pointer, a workspace)."""
    xyz = _cuda("xyz", xyz, (torch.float32, torch.float64), 3).to(torch.float32).contiguous()
    n = int(xyz.shape[0])
    mask_ptr = None
    if mask is not None:
        if _cuda("mask", mask, (torch.bool, torch.uint8)).shape[0] != n:
            raise RuntimeError("mask must have one entry per row of xyz")
        mask = mask.to(torch.uint8).contiguous()
        mask_ptr = mask.data_ptr()
    need = workspace_bytes(n)
    if need < 0:
        _lib.check(-3, "outliers (fewer than 2^31 rows)")
    return xyz, mask, mask_ptr, torch.empty((need,), dtype=torch.uint8, device=xyz.device)


def radius_count(xyz, mask=None, radius=0.04, min_neighbours=16):
    """``xyz`` (N,3) float32 (float64: decided on its float32 rounding) on the GPU, any strides; ``mask`` (N) bool / uint8 or
    None -> ``count`` (N) int32 on the device: min(the other graph rows within ``radius``, ``min_neighbours``), -1 for a row
    outside the graph.  No host read."""
    xyz, mask, mask_ptr, workspace = _inputs(xyz, mask)
    n = int(xyz.shape[0])
    count = torch.empty((n,), dtype=torch.int32, device=xyz.device)
    _lib.call("regnet_outlier_radius_f32", xyz, xyz.data_ptr(), mask_ptr, n, float(radius), int(min_neighbours),
              count.data_ptr(), workspace.data_ptr())
    return count


def knn_mean_distance(xyz, mask=None, k=20, max_radius=0.04):
    """-> ``(mean_dist (N) float32, found (N) int32)`` on the device: ``found`` = min(the other graph rows within
    ``max_radius``, ``k``), -1 outside the graph; ``mean_dist`` = the mean distance to the ``k`` nearest of them where ``found
    == k``, NaN elsewhere.  No host read."""
    xyz, mask, mask_ptr, workspace = _inputs(xyz, mask)
    n = int(xyz.shape[0])
    mean_dist = torch.empty((n,), dtype=torch.float32, device=xyz.device)
    found = torch.empty((n,), dtype=torch.int32, device=xyz.device)
    _lib.call("regnet_outlier_knn_f32", xyz, xyz.data_ptr(), mask_ptr, n, int(k), float(max_radius), mean_dist.data_ptr(),
              found.data_ptr(), workspace.data_ptr())
    return mean_dist, found


def distance_stats(mean_dist, found, k, std_ratio):
    """-> ``stats`` (4) float64 on the device = (n, mu, sigma, threshold) over the rows with ``found == k``: the two-pass
    deviation, float64 sums in a fixed order, threshold = float32(mu + std_ratio * sigma), +inf with fewer than two rows."""
    mean_dist = _cuda("mean_dist", mean_dist, torch.float32).contiguous()
    found = _cuda("found", found, torch.int32).contiguous()
    if found.shape[0] != mean_dist.shape[0]:
        raise RuntimeError("found must have one entry per entry of mean_dist")
    stats = torch.empty((4,), dtype=torch.float64, device=mean_dist.device)
    _lib.call("regnet_outlier_stats_f64", mean_dist, mean_dist.data_ptr(), found.data_ptr(), int(mean_dist.shape[0]), int(k),
              float(std_ratio), stats.data_ptr())
    return stats


def filter_cloud(xyz, params=None, mask=None):
    """``xyz`` (N,3) float32 / float64 on the GPU, ``params`` an ``OutlierParams``, a dict of its fields or None (the defaults),
    ``mask`` (N) bool / uint8 or None -> ``Filtered``.  Everything stays on the device; no host read."""
    p = OutlierParams() if params is None else OutlierParams.coerce(params)
    xyz = _cuda("xyz", xyz, (torch.float32, torch.float64), 3).to(torch.float32).contiguous()
    dev = xyz.device
    status = None
    count = mean_dist = found = stats = None
    if p.mode in ("radius", "both"):
        count = radius_count(xyz, mask, p.radius, p.min_neighbours)
        keep = count == int(p.min_neighbours)
        status = torch.where(keep, KEPT, torch.where(count < 0, NOT_A_ROW, TOO_FEW_IN_RADIUS))
        mask = keep
    if p.mode in ("statistical", "both"):
        mean_dist, found = knn_mean_distance(xyz, mask, p.knn, p.max_radius)
        stats = distance_stats(mean_dist, found, p.knn, p.std_ratio)
        keep = mean_dist <= stats[3].to(torch.float32)        # (a NaN fails)
        second = torch.where(keep, KEPT, torch.where(found < 0, NOT_A_ROW, torch.where(found < int(p.knn), TOO_FEW_NEAREST, TOO_FAR)))
        # "both": the rows the radius stage removed are outside the second stage's graph and keep their first status
        status = second if status is None else torch.where(status == KEPT, second, status)
    status = status.to(torch.uint8)
    num = (status[:, None] == torch.arange(5, dtype=torch.uint8, device=dev)[None, :]).sum(dim=0).to(torch.int32)
    return Filtered(keep, status, num, stats, mean_dist, count, found)
