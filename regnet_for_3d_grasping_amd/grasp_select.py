"""Pose non-maximum suppression + top-K over one grasp set, on the device (csrc/nms.hip): from the up to 4000 collision-free
8-tuples of a set, in which neighbouring region centres regress nearly the same grasp, to the K best DISTINCT ones.

Two grasps are the same grasp when their centres are within ``translation_thresh`` (inclusive) and their frames
(``eval_collision.grasp_frames``: approach, axis_y, minor normal) within ``rotation_thresh_deg`` of one another -- with
``symmetric`` also when one is the other turned by 180 degrees about its approach axis, which a parallel-jaw gripper cannot tell
apart.  The grasps are ranked by descending score (column 7; NaN as -inf, equal scores by lower row), walked in that order, and
one is kept unless an already kept one is the same grasp.  The arithmetic is pinned (DESIGN.md par. 5, include/regnet_hip.h):
``tests/nms_reference.py`` restates it in numpy and the two agree exactly.

``pose_nms`` returns the kept rows; ``pose_nms_device`` returns ``(keep, count)`` on the device with no host read (usable inside
a captured graph).  GPU only: there is no CPU path.
"""
import math
from dataclasses import dataclass
from typing import Optional

import numpy as np
import torch

from . import _lib
from ._frame_util import ParamsBase, require_cuda
from .eval_collision import grasp_frames

_check = _lib.check
_L = _lib.lib

MAX_GRASPS = 32768          # regnet_grasp_nms_f32's documented limit (the pair mask's upper triangle is 64 MiB there)
SOURCES = ("grasp_stage2", "grasp_stage3_stage2", "grasp_stage3", "grasp_stage3_score")


@dataclass
class SelectParams(ParamsBase):
    """What ``GraspDetector(select=...)`` takes (a dict with these keys works too): which of the four collision-filtered grasp
    sets to select from, how many to keep (``None`` / <= 0: every distinct one) and ``pose_nms``'s thresholds."""
    WORD = "select"
    source: str = "grasp_stage3"
    top_k: Optional[int] = None
    translation_thresh: float = 0.03
    rotation_thresh_deg: float = 30.0
    symmetric: bool = True

    def __post_init__(self):
        if self.source not in SOURCES:
            raise ValueError("select: source must be one of %s, not %r" % (", ".join(SOURCES), self.source))

    def nms(self):
        """``pose_nms``'s keywords other than ``top_k``: what the per-frame and the per-object selection share."""
        return {"translation_thresh": self.translation_thresh, "rotation_thresh_deg": self.rotation_thresh_deg,
                "symmetric": self.symmetric}


def thresholds(translation_thresh, rotation_thresh_deg):
    """-> (T2, C) as Python floats holding float32 values: T2 = float32(t) * float32(t) (a float32 product), C = 1 + 2 cos(theta)
    evaluated in float64 and rounded once to float32 (the trace of a rotation by theta)."""
    t = np.float32(translation_thresh)
    return float(np.float32(t * t)), float(np.float32(1.0 + 2.0 * math.cos(math.radians(float(rotation_thresh_deg)))))


def workspace_bytes(n):
    """Bytes of scratch ``regnet_grasp_nms_f32`` needs for ``n`` grasps: nb (nb + 1) / 2 * 64 * 8 with nb = ceil(n / 64)."""
    return int(_L.regnet_grasp_nms_workspace_bytes(int(n)))


def _grasp_ok(grasp):
    require_cuda("grasp", grasp, torch.float32, 8, at_least=True, error=RuntimeError)


def rank_order(score):
    """(n) float32 -> (n) int64: rows by descending score, NaN as -inf, equal scores (-0.0 == 0.0) by lower row."""
    clean = torch.where(torch.isnan(score), torch.full_like(score, float("-inf")), score) + 0.0   # (+ 0.0: -0.0 -> +0.0)
    return torch.sort(clean, descending=True, stable=True).indices


def nms_ranked(center, frame, order, translation_thresh=0.03, rotation_thresh_deg=30.0, top_k=None, symmetric=True,
               keep=None, count=None, workspace=None):
    """The kernels on their own: center (n,3), frame (n,3,3) float32 contiguous, order (n) int64 -> (keep (n) int64, count (1)
    int32) on the device, on the current stream.  ``keep`` / ``count`` / ``workspace`` (uint8, ``workspace_bytes(n)``) may be
    handed in to run without an allocation."""
    for name, x in (("center", center), ("frame", frame), ("order", order)):
        if not x.is_cuda:
            raise RuntimeError("%s must be a CUDA tensor (no CPU path)" % name)
    n = int(center.shape[0])
    if center.dtype != torch.float32 or frame.dtype != torch.float32 or order.dtype != torch.int64 \
            or tuple(center.shape) != (n, 3) or tuple(frame.shape) != (n, 3, 3) or tuple(order.shape) != (n,):
        raise RuntimeError("nms_ranked: center (n,3) / frame (n,3,3) float32 and order (n) int64 expected")
    center, frame, order = center.contiguous(), frame.contiguous(), order.contiguous()
    dev = center.device
    T2, C = thresholds(translation_thresh, rotation_thresh_deg)
    k = 0 if top_k is None else int(top_k)
    if keep is None:
        keep = torch.empty((n,), dtype=torch.int64, device=dev)
    if count is None:
        count = torch.empty((1,), dtype=torch.int32, device=dev)
    if n == 0:
        count.zero_()
        return keep, count
    need = workspace_bytes(n)
    if need < 0:
        _check(-3, "grasp_nms (at most %d grasps)" % MAX_GRASPS)
    if workspace is None:
        workspace = torch.empty((need,), dtype=torch.uint8, device=dev)
    if keep.dtype != torch.int64 or keep.numel() != n or not keep.is_contiguous() or count.dtype != torch.int32 \
            or count.numel() != 1 or workspace.dtype != torch.uint8 or workspace.numel() < need \
            or not workspace.is_contiguous():
        raise RuntimeError("nms_ranked: keep (n) int64, count (1) int32, workspace (>= %d) uint8 expected" % need)
    _lib.call("regnet_grasp_nms_f32", center, center.data_ptr(), frame.data_ptr(), order.data_ptr(), n, T2, C,
              1 if symmetric else 0, k, keep.data_ptr(), count.data_ptr(), workspace.data_ptr())
    return keep, count


def pose_nms_device(grasp, translation_thresh=0.03, rotation_thresh_deg=30.0, top_k=None, symmetric=True, keep=None,
                    count=None, workspace=None):
    """``grasp`` (n, >=8) float32 on the GPU, any strides -> ``(keep, count)``: keep (n) int64 = the rows of the kept grasps in
    rank order followed by -1, count (1) int32, both on the device.  No host read: callable inside a captured graph."""
    _grasp_ok(grasp)
    g8 = grasp[:, :8].contiguous()
    frame, center = grasp_frames(g8)
    order = rank_order(g8[:, 7])
    return nms_ranked(center, frame, order, translation_thresh, rotation_thresh_deg, top_k, symmetric, keep, count,
                      workspace)


def pose_nms(grasp, translation_thresh=0.03, rotation_thresh_deg=30.0, top_k=None, symmetric=True, return_index=False):
    """The best distinct grasps of ``grasp`` (n, >=8) float32 on the GPU: its kept rows, all columns, in rank order (and their
    int64 row numbers with ``return_index``).  One 4-byte read of the kept count at the very end sizes the result."""
    _grasp_ok(grasp)
    if grasp.shape[0] == 0:
        index = torch.empty((0,), dtype=torch.int64, device=grasp.device)
    else:
        keep, count = pose_nms_device(grasp, translation_thresh, rotation_thresh_deg, top_k, symmetric)
        index = keep[:int(count.item())]
    rows = grasp.index_select(0, index)
    return (rows, index) if return_index else rows
