"""Approach analysis against the TSDF volume (csrc/approach_volume.hip): free of seen surfaces and, if asked, of unseen space.

``approach.analyse`` sweeps the hand through the points one cloud holds.  To a point scan the occluded back of an object, the
space behind it and everything no camera has seen look like free space.  The volume (``tsdf.Volume``) knows three states per
voxel -- seen solid (``D < 0``), seen free (observed, ``D >= 0``) and never observed (``W < min_weight``) -- and
``analyse_volume`` holds the swept hand against them: a lattice of samples of the hand in every grasp's local frame, each looked
up in its nearest voxel.  Per grasp it gives

* ``clearance_seen`` / ``clearance_safe``: the longest straight retreat along ``-approach`` on which the hand touches no solid
  voxel / no solid, unobserved or outside voxel, capped at ``standoff``; ``clearance`` is the one ``params.unseen`` names;
* ``width`` / ``offset`` / ``opening``: as ``approach.Approach``, from the solid samples between the fingers -- the fused model,
  not one view's cloud;
* ``unseen_share``: the share of the swept hand's samples that lie in unseen space; ``solid_hand``: the samples of the hand at
  its final pose that are solid;
* ``contact``: with ``friction_deg`` and a ``tsdf.Surface``, ``approach``'s contact check on the surface's rows and the normals
  of the volume's gradient -- no normal is estimated from a cloud here; 0 without a surface.

Every value is a sample's coordinate: quantised to the lattice step, and the lookup is the nearest voxel, not an interpolation.
The arithmetic is pinned (include/regnet_hip.h), so ``tests/approach_volume_reference.py`` restates it in numpy and the two agree
exactly.  Nothing here reads from the device or waits for it.  GPU only: there is no CPU path.
"""
import math

import numpy as np
import torch

from . import _lib, approach, eval_collision
from ._frame_util import matrix4, require_cuda, to_device

MAX_SAMPLES = 1 << 22               # regnet_grasp_approach_volume_f32's documented limit on the lattice


def lattice(box, standoff, step, x_extent):
    """The samples per axis of a call -> (n_x, n_y, n_z): ``max(1, ceil(extent / h))`` in float64 from the float32 constants, as
    the entry point evaluates them.  ``box``: ``eval_collision._box_args``' tuple."""
    x_lo, ht, hw = np.float32(box[0]), np.float32(box[3]), np.float32(box[4])
    h = float(np.float32(step))
    xs = np.float32(x_lo - np.float32(standoff))
    extents = (float(np.float32(x_extent)) - float(xs), float(hw) + float(hw), float(ht) + float(ht))
    return tuple(max(1, int(math.ceil(e / h))) for e in extents)


class VolumeApproach(approach.Approach):
    """``analyse_volume``'s result, all on the device.  ``counts`` (B,8) int32 = (region SOLID, region UNSEEN, hand SOLID, hand
    UNSEEN, blockers SOLID, blockers UNSEEN, memberships, memberships OUTSIDE) and ``values`` (B,4) float32 = (y_min, y_max,
    clearance_seen, clearance_safe) are the kernel's; ``contact_counts`` (B,8) int32 is ``regnet_grasp_approach_f32``'s on the
    surface, or None; ``L`` (B,12) / ``T`` (B,4,4) float32 are the local-to-volume rows the kernel was given and the
    volume-to-local matrices of the contact pass (None without it); ``samples`` = (n_x, n_y, n_z).  With a ``field``:
    ``margins`` (B,2) int32 and ``margin_counts`` (B,4) int32 are ``regnet_grasp_margin_volume_f32``'s, else None; with a SIGNED
    field they are ``regnet_grasp_margin_volume_signed_f32``'s, ``margin_counts`` (B,6).  ``width``, ``offset``,
    ``opening``, ``pregrasp`` and ``passes()`` are ``Approach``'s, on the solid samples and the policy's clearance."""

    def __init__(self, counts, values, frame, center, params, half_space, contact_counts, L, T, samples, margins=None,
                 margin_counts=None, margin_metres=None):
        super().__init__(counts, values, frame, center, params, half_space)
        self.contact_counts, self.L, self.T, self.samples = contact_counts, L, T, samples
        self.margins, self.margin_counts, self._margin_metres = margins, margin_counts, margin_metres
        self.retreat = None                       # the ``retreat.RetreatFan`` of ``params.retreat``, set by ``analyse_volume``
        self.paths = None                         # the ``hand_path.PathCheck`` of ``params.paths``, set by ``analyse_volume``
        self.push = None                          # the ``hand_adjust.PushOut`` of ``params.push``, set by ``analyse_volume``:
                                                  # ``center`` and ``L`` are then the MOVED ones of the grasps it freed

    @property
    def margin_hand(self):
        """(B) float32 [m]: the distance from the hand at its final pose (the samples behind the palm face and inside the
        fingers) to the nearest obstacle of the ``field`` given to ``analyse_volume``, ``+inf`` when the field has no obstacle or
        the hand no sample; None without a field.  Not the SOLID threshold ``params.margin``."""
        return None if self._margin_metres is None else self._margin_metres[0]

    @property
    def margin_sweep(self):
        """(B) float32 [m]: the same over the whole swept hand, so ``margin_sweep <= margin_hand``; None without a field."""
        return None if self._margin_metres is None else self._margin_metres[1]

    @property
    def colliding_hand(self):
        """(B) int32: the hand samples with a negative value of a SIGNED field -- inside an obstacle, or outside a volume whose
        outside counts as one; None without a signed field.  ``margin_hand`` is then negative: minus the penetration depth."""
        return self.margin_counts[:, 4] if self.margin_counts is not None and self.margin_counts.shape[1] == 6 else None

    @property
    def colliding_sweep(self):
        """(B) int32: the same over the whole swept hand; None without a signed field."""
        return self.margin_counts[:, 5] if self.margin_counts is not None and self.margin_counts.shape[1] == 6 else None

    def passes(self):
        """``Approach.passes()``, and ``margin_hand >= min_margin`` and the retreat fan's ``free_length >= min_retreat`` when
        those are set, compared as float32."""
        ok = super().passes()
        if self.params.min_margin is not None:
            if self._margin_metres is None:
                raise ValueError("approach: min_margin needs a distance field; give analyse_volume field=...")
            ok = ok & (self.margin_hand >= float(np.float32(self.params.min_margin)))
        if self.params.min_retreat is not None:
            if self.retreat is None:
                raise ValueError("approach: min_retreat needs the retreat fan; give analyse_volume field=... and params.retreat")
            ok = ok & self.retreat.passes(self.params.min_retreat)
        if self.params.min_path is not None:      # the picked path's CERTIFIED length, compared as float32
            if self.paths is None:
                raise ValueError("approach: min_path needs the hand paths; give analyse_volume field=... and params.paths")
            ok = ok & (self.paths.certified_length >= float(np.float32(self.params.min_path)))
        if self.params.push is not None and self.params.push_keep == "freed":
            if self.push is None:
                raise ValueError("approach: push_keep needs the push-out; give analyse_volume field=... and params.push")
            ok = ok & self.push.freed()
        return ok

    @property
    def clearance_seen(self):
        return self.values[:, 2]

    @property
    def clearance_safe(self):
        return self.values[:, 3]

    @property
    def clearance(self):
        """``clearance_seen``, or ``clearance_safe`` with ``unseen="blocked"``."""
        return self.clearance_safe if self.params.unseen == "blocked" else self.clearance_seen

    @property
    def solid_hand(self):
        """(B) int32: the solid samples behind the palm face and inside the fingers at the final pose."""
        return self.counts[:, 2]

    @property
    def unseen_share(self):
        """(hand UNSEEN + blockers UNSEEN) / memberships as float32, 0 where there is no sample."""
        share = (self.counts[:, 3] + self.counts[:, 5]).to(torch.float32) / self.counts[:, 6].to(torch.float32)
        return torch.where(self.counts[:, 6] == 0, torch.zeros_like(share), share)

    @property
    def contact(self):
        """(ok_left / n_left) * (ok_right / n_right) on the surface's rows, 0 where either band is empty or without a surface."""
        if self.contact_counts is None:
            return torch.zeros((self.counts.shape[0],), dtype=torch.float32, device=self.counts.device)
        c = self.contact_counts.to(torch.float32)
        share = (c[:, 4] / c[:, 3]) * (c[:, 6] / c[:, 5])
        return torch.where((self.contact_counts[:, 3] == 0) | (self.contact_counts[:, 5] == 0), torch.zeros_like(share), share)


def _rows_times(rows, matrix):
    """``rows`` (B,4,4) float64 times the host 4x4 ``matrix`` -> (B,4,4) float64, entry (r, c) = ((rows[r,0] m[0,c] + rows[r,1]
    m[1,c]) + rows[r,2] m[2,c]) + rows[r,3] m[3,c]: elementwise, no BLAS, nothing uploaded."""
    return torch.stack([((rows[:, :, 0] * float(matrix[0, c]) + rows[:, :, 1] * float(matrix[1, c]))
                         + rows[:, :, 2] * float(matrix[2, c])) + rows[:, :, 3] * float(matrix[3, c]) for c in range(4)], dim=2)


def _times_rows(matrix, rows):
    """The host 4x4 ``matrix`` times ``rows`` (B,4,4) float64 -> (B,4,4) float64, in the same order of operations."""
    return torch.stack([((rows[:, 0, :] * float(matrix[r, 0]) + rows[:, 1, :] * float(matrix[r, 1]))
                         + rows[:, 2, :] * float(matrix[r, 2])) + rows[:, 3, :] * float(matrix[r, 3]) for r in range(4)], dim=1)


def local_to_volume(grasp, to_volume):
    """``grasp`` (B, >=8) float32 on the device, ``to_volume`` a 4x4 or None (identity) -> (the 4x4 as a float64 host array,
    ``frame`` (B,3,3), ``center`` (B,3), ``L`` (B,12) float32): ``L = to_volume @ [frame | centre]`` per grasp, formed on the
    device in float64 and rounded once -- the rows ``analyse_volume`` and ``retreat.retreat_fan`` hand to their kernels."""
    B, dev = int(grasp.shape[0]), grasp.device
    to_volume = np.eye(4) if to_volume is None else matrix4(to_volume, "to_volume must be a finite 4x4 transform", finite=True)
    frame, center = eval_collision.grasp_frames(grasp[:, :8].contiguous())
    local = torch.zeros((B, 4, 4), dtype=torch.float64, device=dev)
    local[:, :3, :3] = frame
    local[:, :3, 3] = center
    local[:, 3, 3] = 1.0
    L = _times_rows(to_volume, local)[:, :3, :].reshape(B, 12).to(torch.float32).contiguous()
    return to_volume, frame, center, L


def hand_call(who, volume, grasp, depth, max_depth):
    """The opening of every function that holds the hand's sample lattice against ``volume`` or its distance field (``who``: its
    name, for the messages): the grasps are (B, >=8) float32 on the volume's device, and a depth per grasp needs ``max_depth`` and
    goes to the device.  -> (the device, B, ``depth``, ``x_extent``: the far end of the lattice).  The caller's own rules and
    its rows come next, then ``hand_lattice``."""
    require_cuda("grasp", grasp, torch.float32, 8, at_least=True, error=RuntimeError)
    dev = volume.device
    if grasp.device != dev:
        raise RuntimeError("%s: the grasps are on %s, the volume on %s" % (who, grasp.device, dev))
    per_grasp = (isinstance(depth, torch.Tensor) and depth.dim() > 0) or (not isinstance(depth, torch.Tensor) and np.ndim(depth) > 0)
    if per_grasp and max_depth is None:
        raise ValueError("%s: with one depth per grasp give max_depth, the far end of the sample lattice" % who)
    if per_grasp and not isinstance(depth, torch.Tensor):
        depth = to_device(np.asarray(depth, dtype=np.float32), dev)
    return dev, int(grasp.shape[0]), depth, float(max_depth) if per_grasp else float(depth)


def hand_lattice(who, volume, depth, width, B, step, standoff, x_extent):
    """The box and the lattice of a call that ``hand_call`` opened -> (``eval_collision._box_args``' tuple, the tensor it points
    into -- keep it until the launch --, the step [m], (n_x, n_y, n_z)).  ``step``: None is the volume's voxel; ``standoff``: how
    far the hand is swept, None for the hand at its final pose.  More than 2^22 samples are a ValueError."""
    box, keep = eval_collision._box_args(depth, width, B, volume.device)
    step = float(volume.params.voxel) if step is None else float(step)
    samples = lattice(box, 0.0 if standoff is None else standoff, step, x_extent)
    if samples[0] * samples[1] * samples[2] > MAX_SAMPLES:
        raise ValueError("%s: %d x %d x %d samples of the %s, more than 2^22; raise step"
                         % ((who,) + samples + ("hand" if standoff is None else "swept hand",)))
    return box, keep, step, samples


def require_field(who, volume, field):
    """``field`` must be a ``tsdf.DistanceField`` of ``volume`` -- the same dims, on its device -- else a ValueError."""
    if not (hasattr(field, "dist2") and hasattr(field, "metres")) or tuple(field.dims) != tuple(volume.params.dims) \
            or field.dist2.device != volume.device:
        raise ValueError("%s: the field must be a DistanceField of this volume (same dims, same device)" % who)


def analyse_volume(volume, grasp, depth, width, params=None, to_volume=None, surface=None, max_depth=None, field=None):
    """``volume``: a ``tsdf.Volume``; ``grasp`` (B, >=8) float32 on its device; ``depth``: a float or one depth per grasp -- then
    ``max_depth``, a bound on them, is the lattice's far end (nothing is read back to find it; a ValueError without it);
    ``width``: the gripper's opening; ``params``: ``ApproachParams`` / a dict / None -- ``standoff``, ``unseen``, ``step``,
    ``margin``, ``pad``, ``friction_deg``, ``contact_depth``, ``min_clearance`` and ``min_contact`` are read; ``to_volume``: the
    4x4 that takes the grasps' frame to the volume's (None: identity); ``surface``: a ``tsdf.Surface`` of the volume, for the
    contact check.  -> ``VolumeApproach``.

    ``L = to_volume @ [frame | centre]`` per grasp is formed on the device in float64 and rounded once; the kernel takes it as
    an input.  The contact pass runs ``regnet_grasp_approach_f32`` on ``surface.xyz`` / ``surface.normal`` with ``T = [frame^T |
    -frame^T centre] @ inverse(to_volume)``, float64 rounded once -- the inverse of ``L`` with the frame's transpose for its
    inverse and ``to_volume`` inverted on the host.  One launch (two with the contact pass) on the current stream, no host
    read.

    ``field``: a ``tsdf.DistanceField`` of the same volume (``volume.distance_field(...)``); the same lattice and ``L`` are then
    also read against it (``regnet_grasp_margin_volume_f32``, one more launch and a conversion to metres) and the result has
    ``margin_hand`` / ``margin_sweep``.  Nothing else of the result changes.  A SIGNED field (``distance_field(signed=True)``)
    is read by ``regnet_grasp_margin_volume_signed_f32``: ``margin_hand`` / ``margin_sweep`` are signed metres, a negative value
    minus the penetration depth of the deepest sample, ``colliding_hand`` / ``colliding_sweep`` count the samples inside an
    obstacle, and ``min_margin`` judges the signed value.  With ``params.retreat`` and a field the result's ``retreat`` is
    ``retreat.retreat_fan``'s ``RetreatFan`` of the same grasps (two launches more, on the ``L`` formed here); None without
    ``params.retreat``, and ``params.retreat`` without a field is a ValueError.  ``params.paths`` (``approach.PathApproachParams``)
    likewise sets the result's ``paths`` to ``hand_path.check_paths``' ``PathCheck``.

    ``params.push`` (``approach.PushApproachParams``; it needs a signed, capped field) runs ``hand_adjust.push_out`` on the grasps
    FIRST, one launch, and sets the result's ``push`` to its ``PushOut``.  A grasp it FREED is then analysed -- everything above:
    classification, margins, contact, fan and paths -- at its moved centre: its row of ``L`` is the push-out's ``pose`` and its
    row of the result's ``center`` is ``PushOut.moved_centres``'.  Every other grasp is analysed as it came, whatever the
    push-out made of it.  The choice is a ``torch.where`` on the device: still no host read."""
    params = approach.ApproachParams.coerce(params) or approach.ApproachParams()
    if params.retreat is not None and field is None:
        raise ValueError("analyse_volume: params.retreat reads a distance field; give field=volume.distance_field(...)")
    if params.paths is not None and field is None:
        raise ValueError("analyse_volume: params.paths reads a distance field; give field=volume.distance_field(...)")
    if params.push is not None and field is None:
        raise ValueError("analyse_volume: params.push follows a distance field; give field=volume.distance_field(signed=True, "
                         "max_distance=...)")
    p = volume.params
    dev, B, depth, x_extent = hand_call("analyse_volume", volume, grasp, depth, max_depth)
    to_volume, frame, center, L = local_to_volume(grasp, to_volume)
    pushed = None
    if params.push is not None:                   # first: the grasps it frees are analysed where it left them
        from . import hand_adjust
        pushed = hand_adjust.push_out(volume, field, grasp, depth, width, params.push, to_volume, max_depth, rows=(frame, center, L))
        moved = pushed.moved().unsqueeze(1)
        L = torch.where(moved, pushed.pose, L).contiguous()
        center = torch.where(moved, pushed.moved_centres(center, frame).to(center.dtype), center)
    box, keep, step, samples = hand_lattice("analyse_volume", volume, depth, width, B, params.step, params.standoff, x_extent)
    nx, ny, nz = p.dims
    counts = torch.empty((B, 8), dtype=torch.int32, device=dev)
    values = torch.empty((B, 4), dtype=torch.float32, device=dev)
    _lib.call("regnet_grasp_approach_volume_f32", volume.data, volume.data.data_ptr(), nx, ny, nz, volume.origin.ctypes.data,
              float(p.voxel), float(p.trunc), int(p.min_weight), float(params.margin), L.data_ptr(), B, *box,
              float(params.standoff), step, x_extent, counts.data_ptr(), values.data_ptr())
    margins = margin_counts = margin_metres = None
    if field is not None:
        require_field("analyse_volume", volume, field)
        margins = torch.empty((B, 2), dtype=torch.int32, device=dev)
        signed = field.signed
        margin_counts = torch.empty((B, 6 if signed else 4), dtype=torch.int32, device=dev)
        entry = "regnet_grasp_margin_volume_signed_f32" if signed else "regnet_grasp_margin_volume_f32"
        _lib.call(entry, field.dist2, field.dist2.data_ptr(), nx, ny, nz, volume.origin.ctypes.data, float(p.voxel), int(field.outside), L.data_ptr(), B, *box, float(params.standoff), step, x_extent,
                  margins.data_ptr(), margin_counts.data_ptr())
        margin_metres = field.metres(margins.t().contiguous())      # (2,B): row 0 the hand, row 1 the sweep
    contact_counts = T = None
    if params.friction_deg is not None and surface is not None:
        points = require_cuda("surface.xyz", surface.xyz, torch.float32, 3, error=RuntimeError)
        normals = require_cuda("surface.normal", surface.normal, torch.float32, 3, error=RuntimeError)
        if normals.shape[0] != points.shape[0] or points.device != dev or normals.device != dev:
            raise RuntimeError("analyse_volume: the surface must have one normal per row, on the volume's device")
        inverse = torch.zeros((B, 4, 4), dtype=torch.float64, device=dev)
        turned = frame.to(torch.float64).transpose(1, 2)
        inverse[:, :3, :3] = turned
        c = center.to(torch.float64)
        inverse[:, :3, 3] = -((turned[:, :, 0] * c[:, 0:1] + turned[:, :, 1] * c[:, 1:2]) + turned[:, :, 2] * c[:, 2:3])
        inverse[:, 3, 3] = 1.0
        T = _rows_times(inverse, np.linalg.inv(to_volume)).to(torch.float32).contiguous()
        contact_counts = torch.empty((B, 8), dtype=torch.int32, device=dev)
        contact_values = torch.empty((B, 4), dtype=torch.float32, device=dev)
        _lib.call("regnet_grasp_approach_f32", points, points.data_ptr(), points.stride(0), points.stride(1), normals.data_ptr(),
                  normals.stride(0), normals.stride(1), int(points.shape[0]), T.data_ptr(), B, *box, float(params.standoff),
                  float(params.contact_depth), approach.cos_friction(params.friction_deg), contact_counts.data_ptr(),
                  contact_values.data_ptr())
    result = VolumeApproach(counts, values, frame, center, params, box[5], contact_counts, L, T, samples, margins, margin_counts,
                            margin_metres)
    result.push = pushed
    if params.retreat is not None:
        from . import retreat
        result.retreat = retreat.retreat_fan(volume, field, grasp, depth, width, params.retreat, to_volume, max_depth,
                                             rows=(frame, center, L))
    if params.paths is not None:                  # (``approach.PathApproachParams``) the same grasps through posed paths
        from . import hand_path
        result.paths = hand_path.check_paths(volume, field, grasp, depth, width, params.paths, to_volume, max_depth,
                                             rows=(frame, center, L))
    return result
