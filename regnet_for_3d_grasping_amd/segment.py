"""Object segmentation on the device (csrc/cluster.hip): which object a point, and a grasp, belongs to.

``cluster_points`` is Euclidean cluster extraction -- the connected components of the graph "squared distance <= tolerance^2"
over the rows of a cloud that a mask keeps and whose coordinates are finite.  Components of at least ``min_points`` rows are
kept, ranked by descending size (equal sizes by their smallest row), and the first ``max_objects`` of them are the objects:
``label`` per row, ``size`` / ``first`` / ``bbox`` per object.  ``assign_grasps`` gives every grasp the object of the nearest
labelled point within ``radius`` of its centre; ``select_per_object`` takes the ``k`` best distinct grasps of every object out of
one pose NMS over the whole set.  The arithmetic is pinned (include/regnet_hip.h, DESIGN.md par. 5): float32, every operation
rounded on its own, so ``tests/cluster_reference.py`` restates it in numpy and the two agree exactly.

Nothing here reads from the device except ``Segmentation.objects()``; nothing draws from numpy's random stream.  GPU only: there
is no CPU path.
"""
from dataclasses import dataclass
from typing import Optional

import numpy as np
import torch

from . import _lib, grasp_select
from ._frame_util import ParamsBase, require_cuda

_L = _lib.lib


@dataclass
class SegmentParams(ParamsBase):
    """What ``GraspDetector(segment=...)`` takes (a dict with these keys works too).  ``tolerance``: two points this close [m]
    belong to one object; ``min_points``: smaller clusters are dropped; ``max_objects``: the largest so many are kept;
    ``table_clearance``: points must lie this far above the table; ``assign_radius``: a grasp belongs to the object of the
    nearest object point within this distance of its centre; ``source``: the grasp set that is assigned (None: the ``select``
    source, else ``"grasp_stage3"``); ``top_k_per_object``: None, or how many distinct grasps to select for every object -- the
    per-object selection then REPLACES the per-frame one: of a ``select`` given as well, the source and the NMS thresholds are
    used and ``top_k`` is not.

    The defaults are a choice made from the reference's gripper (8 cm opening, 6 cm fingers) and crop sizes.  Nobody has
    measured them on real frames."""
    WORD = "segment"
    tolerance: float = 0.01
    min_points: int = 50
    max_objects: int = 64
    table_clearance: float = 0.01
    assign_radius: float = 0.03
    source: Optional[str] = None
    top_k_per_object: Optional[int] = None

    def __post_init__(self):
        if self.source is not None and self.source not in grasp_select.SOURCES:
            raise ValueError("segment: source must be None or one of %s, not %r" % (", ".join(grasp_select.SOURCES), self.source))
        if not (float(self.tolerance) > 0.0 and np.isfinite(self.tolerance)):
            raise ValueError("segment: tolerance must be positive and finite")
        if int(self.min_points) < 1 or int(self.max_objects) < 1:
            raise ValueError("segment: min_points and max_objects must be at least 1")
        if not np.isfinite(self.table_clearance):
            raise ValueError("segment: table_clearance must be finite")
        if not (float(self.assign_radius) >= 0.0 and np.isfinite(self.assign_radius)):
            raise ValueError("segment: assign_radius must be non-negative and finite")
        if self.top_k_per_object is not None and int(self.top_k_per_object) < 1:
            raise ValueError("segment: top_k_per_object must be None or at least 1")


class Segmentation:
    """``cluster_points``' result, all on the device: ``root`` (N) int32 = the smallest row of the row's component or -1,
    ``label`` (N) int32 = its object or -1, ``num`` (2) int32 = (objects, kept components), ``size`` / ``first`` (max_objects)
    int32 and ``bbox`` (max_objects, 6) float32 = (min x, y, z, max x, y, z), filled for the first ``num[0]`` objects."""

    def __init__(self, root, label, num, size, first, bbox):
        self.root, self.label, self.num, self.size, self.first, self.bbox = root, label, num, size, first, bbox

    def objects(self):
        """The one blocking read: ``num`` and the three tables in a single transfer -> (count, kept, size (count,) int32,
        first (count,) int32, bbox (count, 6) float32) with numpy arrays."""
        k = int(self.size.shape[0])
        packed = torch.cat((self.num, self.size, self.first, self.bbox.reshape(-1).view(torch.int32))).cpu().numpy()
        count, kept = int(packed[0]), int(packed[1])
        size, first = packed[2:2 + k], packed[2 + k:2 + 2 * k]
        bbox = packed[2 + 2 * k:].view(np.float32).reshape(k, 6)
        return count, kept, size[:count].copy(), first[:count].copy(), bbox[:count].copy()


def workspace_bytes(n, max_objects):
    """Bytes of scratch ``regnet_cluster_points_f32`` needs for ``n`` rows."""
    return int(_L.regnet_cluster_workspace_bytes(int(n), int(max_objects)))


def _cuda(name, x, dtype=None, cols=None, at_least=False):
    """Every argument check of this module is a RuntimeError."""
    return require_cuda(name, x, dtype, cols, at_least, error=RuntimeError)


def cluster_points(xyz, mask=None, tolerance=0.01, min_points=50, max_objects=64):
    """``xyz`` (N,3) float32 on the GPU, any strides; ``mask`` (N) bool / uint8 or None -> ``Segmentation``.  Two launches of
    the kernels with one ``torch.sort`` of the component sizes between them; no host read."""
    xyz = _cuda("xyz", xyz, torch.float32, 3).contiguous()
    n, k = int(xyz.shape[0]), int(max_objects)
    dev = xyz.device
    mask_ptr = 0
    if mask is not None:
        if _cuda("mask", mask, (torch.bool, torch.uint8)).shape[0] != n:
            raise RuntimeError("mask must have one entry per row of xyz")
        mask = mask.to(torch.uint8).contiguous()
        mask_ptr = mask.data_ptr()
    need = workspace_bytes(n, k)
    if need < 0:
        _lib.check(-3, "cluster_points (fewer than 2^31 rows, at least one object)")
    workspace = torch.empty((need,), dtype=torch.uint8, device=dev)
    root = torch.empty((n,), dtype=torch.int32, device=dev)
    key = torch.empty((n,), dtype=torch.int32, device=dev)
    label = torch.empty((n,), dtype=torch.int32, device=dev)
    num = torch.empty((2,), dtype=torch.int32, device=dev)
    size = torch.empty((k,), dtype=torch.int32, device=dev)
    first = torch.empty((k,), dtype=torch.int32, device=dev)
    bbox = torch.empty((k, 6), dtype=torch.float32, device=dev)

    def launch(stages, order_ptr):
        _lib.call("regnet_cluster_points_f32", xyz, xyz.data_ptr(), mask_ptr, n, float(tolerance), int(min_points), k,
                  root.data_ptr(), key.data_ptr(), order_ptr, label.data_ptr(), num.data_ptr(), size.data_ptr(),
                  first.data_ptr(), bbox.data_ptr(), workspace.data_ptr(), stages)

    launch(1, 0)
    # the ranking: key's index is the component's root, so a stable descending sort is "size descending, then smaller root"
    order = torch.sort(key, descending=True, stable=True).indices
    launch(2, order.data_ptr())
    return Segmentation(root, label, num, size, first, bbox)


def assign_grasps(grasp, xyz, label, radius=0.03):
    """``grasp`` (Q, >=3) float32 (the centre is columns 0:3), ``xyz`` (N,3) float32, ``label`` (N) int32, all on the GPU ->
    ``(object (Q) int32, point (Q) int32)`` on the device: the nearest labelled row within ``radius`` of the centre and its
    object, -1 without one."""
    query = _cuda("grasp", grasp, torch.float32, 3, at_least=True)[:, :3].contiguous()
    xyz = _cuda("xyz", xyz, torch.float32, 3).contiguous()
    label = _cuda("label", label, torch.int32).contiguous()
    if label.shape[0] != xyz.shape[0]:
        raise RuntimeError("label must have one entry per row of xyz")
    q = int(query.shape[0])
    obj = torch.empty((q,), dtype=torch.int32, device=query.device)
    point = torch.empty((q,), dtype=torch.int32, device=query.device)
    _lib.call("regnet_cluster_assign_f32", query, query.data_ptr(), q, xyz.data_ptr(), label.data_ptr(), int(xyz.shape[0]),
              float(radius), obj.data_ptr(), point.data_ptr())
    return obj, point


def above_table_mask(points32, table_height, clearance):
    """(N,3) float32 -> (N) bool: ``z > float32(float32(table_height) + float32(clearance))``, compared as float32."""
    _cuda("points32", points32, torch.float32, 3, at_least=True)
    level = np.float32(np.float32(table_height) + np.float32(clearance))
    return points32[:, 2] > float(level)


def select_per_object(grasp, object, num_objects, k, **nms):
    """The ``k`` best distinct grasps of every object: one ``grasp_select.pose_nms_device`` over the whole set (``nms``: its
    thresholds; ``top_k`` is not one of them), then of the kept rows, in rank order, the first ``k`` of each object id in
    [0, num_objects), ordered by object id and then by rank.  -> ``(rows, index (m) int64, object_of_row (m) int32)``; the one
    host read sizes the result."""
    if "top_k" in nms:
        raise TypeError("select_per_object: top_k is not a keyword (the NMS runs over the whole set)")
    n = int(grasp.shape[0])
    if tuple(_cuda("object", object).shape) != (n,):
        raise RuntimeError("object must have one entry per grasp")
    grasp_select._grasp_ok(grasp)
    if n == 0:
        index = torch.empty((0,), dtype=torch.int64, device=grasp.device)
        return grasp.index_select(0, index), index, object.to(torch.int32)[index]
    keep, count = grasp_select.pose_nms_device(grasp, top_k=None, **nms)
    rank = torch.arange(n, device=grasp.device)
    kept = rank < count.to(torch.int64)
    obj = torch.where(kept, object.to(torch.int64)[keep.clamp(min=0)], torch.full_like(keep, -1))
    usable = (obj >= 0) & (obj < int(num_objects))
    # rank within the object: sort the usable ranks by object (stable: rank order survives), number each run from 0
    sort_key = torch.where(usable, obj, torch.full_like(obj, int(num_objects)))
    by_object = torch.sort(sort_key, stable=True)
    sorted_obj, sorted_rank = by_object.values, by_object.indices
    run_start = torch.searchsorted(sorted_obj, sorted_obj, right=False)
    taken = (sorted_obj < int(num_objects)) & (rank - run_start < int(k))
    chosen = sorted_rank[taken]
    index = keep[chosen]
    return grasp.index_select(0, index), index, obj[chosen].to(torch.int32)
