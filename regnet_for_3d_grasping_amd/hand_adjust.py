"""Push-out (csrc/hand_adjust.hip): a colliding hand moved free along the signed distance field's gradient.

``analyse_volume`` reports ``margin_hand`` and ``colliding_hand``; the retreat fan and the hand paths report how a hand gets away
from its final pose.  All of them judge a grasp and can only drop it.  ``push_out`` MOVES the rigid hand of every grasp by a
translation -- the rotation is kept -- until its interpolated signed margin reaches a target: at every iterate it finds the hand
sample that lies deepest in the field and steps along the field's gradient there by the distance that is missing (deepest-sample
projection).  A finger 3 mm inside the object, or a palm that touches the table, becomes a grasp shifted by those 3 mm.

The arithmetic is pinned (include/regnet_hip.h "push-out"), so ``tests/hand_adjust_reference.py`` restates it in numpy and the
two agree exactly.  One launch on the current stream, the iteration inside the kernel; nothing here reads from the device or
waits for it.  GPU only: there is no CPU path.
"""
from dataclasses import dataclass
from typing import Any, Optional

import numpy as np
import torch

from . import _lib, approach_volume
from ._frame_util import ParamsBase, check_step

__all__ = ["PushParams", "PushOut", "push_out", "STATUS", "MAX_ITERATIONS"]

MAX_ITERATIONS = 64                 # regnet_grasp_push_out_f32's documented limit on T
# info[:, 0], include/regnet_hip.h's REGNET_PUSH_*
ALREADY_FREE, FREED, MAX_ITER, CAPPED, STUCK, LEFT_VOLUME = range(6)
STATUS = ("ALREADY_FREE", "FREED", "MAX_ITER", "CAPPED", "STUCK", "LEFT_VOLUME")


@dataclass
class PushParams(ParamsBase):
    """What ``push_out`` takes (a dict with these keys works too).  ``target``: the signed margin the hand is to reach [m]
    (0: just out of every obstacle; negative: a tolerated penetration); ``max_shift``: the longest move of the hand [m] -- a step
    that would pass it is not taken; ``iterations``: the most steps (1..64); ``axes``: a factor per LOCAL axis of the hand --
    approach, closing, thickness -- on every step: ``(1, 1, 1)`` moves freely, ``(0, 1, 0)`` re-centres along the closing axis
    only; ``step``: the distance between two samples of the hand [m]; None: the volume's voxel.

    The margin is judged as ``margin >= target`` in float32, without slack: a hand can end MAX_ITER a few nanometres short of
    the target, where a step is below the resolution of the pose's translation (DESIGN.md par. 10); more ``iterations`` let the
    local shift accumulate it, and cost nothing for the hands that end earlier.

    The defaults -- 2 mm of clearance, a move of at most 1 cm, 8 steps -- are choices, unmeasured: nobody has measured them on a
    robot."""
    WORD = "push"
    target: float = 0.002
    max_shift: float = 0.01
    iterations: int = 8
    axes: Any = (1.0, 1.0, 1.0)
    step: Optional[float] = None

    def __post_init__(self):
        with np.errstate(over="ignore", under="ignore"):
            if not np.isfinite(np.float32(self.target)):
                raise ValueError("push: target must be finite in float32")
            if not (float(self.max_shift) >= 0.0 and np.isfinite(np.float32(self.max_shift))):
                raise ValueError("push: max_shift must be non-negative and finite in float32")
        if isinstance(self.iterations, bool) or int(self.iterations) != self.iterations or not 1 <= int(self.iterations) <= MAX_ITERATIONS:
            raise ValueError("push: iterations must be an integer in 1..%d" % MAX_ITERATIONS)
        axes = np.asarray(self.axes, dtype=np.float64)
        with np.errstate(over="ignore"):
            if axes.shape != (3,) or not np.isfinite(axes.astype(np.float32)).all():
                raise ValueError("push: axes must be 3 numbers, finite in float32")
        check_step("push", self.step)


class PushOut:
    """``push_out``'s result, all on the device.  ``pose`` (B,12) float32: the three rows of the hand's local-to-volume matrix
    after the move (``L``'s own where no step was applied); ``shift`` (B,3) float32: the move in the hand's LOCAL frame;
    ``info`` (B,4) int32 = (status, steps applied, the worst sample's index at the last evaluation or -1, the OUTSIDE lookups
    there) and ``trace`` (B, iterations + 1) float32, the margin at every evaluated iterate (NaN at the others), are the
    kernel's; ``L`` (B,12) the rows it started from."""

    def __init__(self, pose, shift, info, trace, L, params):
        self.pose, self.shift, self.info, self.trace, self.L, self.params = pose, shift, info, trace, L, params

    @property
    def status(self):
        """(B) int32: an index into ``STATUS``."""
        return self.info[:, 0]

    @property
    def iterations(self):
        """(B) int32: the steps that were applied."""
        return self.info[:, 1]

    @property
    def margin(self):
        """(B) float32 [m]: the hand's interpolated signed margin at the last evaluated iterate -- at ``pose`` --, ``+inf`` for a
        hand without a sample or without a sample inside the volume."""
        at = self.info[:, 1].to(torch.int64).view(-1, 1)
        return torch.gather(self.trace, 1, at).reshape(-1)

    def freed(self):
        """(B) bool: the hand has the target margin at ``pose``: ALREADY_FREE or FREED."""
        return self.info[:, 0] <= FREED

    def moved(self):
        """(B) bool: FREED -- the hand has the target margin at a pose that is not the one it came with."""
        return self.info[:, 0] == FREED

    def moved_centres(self, centres, rotations):
        """``centres`` (B,3) and ``rotations`` (B,3,3), ``eval_collision.grasp_frames``' of these grasps -> (B,3) float32: the
        centres plus the rotated local shift, ``c_i + ((R_i0 s_0 + R_i1 s_1) + R_i2 s_2)``, in float64 and rounded once.  Not
        pinned bit for bit (the kernel's own result is ``pose``)."""
        R, s = rotations.to(torch.float64), self.shift.to(torch.float64)
        move = (R[:, :, 0] * s[:, 0:1] + R[:, :, 1] * s[:, 1:2]) + R[:, :, 2] * s[:, 2:3]
        return (centres.to(torch.float64) + move).to(torch.float32)


def push_out(volume, field, grasp, depth, width, params=None, to_volume=None, max_depth=None, rows=None):
    """``volume``, ``field``, ``grasp``, ``depth``, ``width``, ``to_volume``, ``max_depth`` and ``rows`` as in
    ``hand_path.check_paths`` (``L`` is formed as it forms it); ``params``: ``PushParams`` / a dict / None (the defaults).
    -> ``PushOut``.  The field must be SIGNED -- an unsigned field has no inside to push out of -- and CAPPED
    (``distance_field(signed=True, max_distance=...)``): an uncapped field has infinite corners, between which nothing can be
    interpolated.  One launch on the current stream, no host read: capturable."""
    params = PushParams.coerce(params) or PushParams()
    p = volume.params
    dev, B, depth, x_extent = approach_volume.hand_call("push_out", volume, grasp, depth, max_depth)
    approach_volume.require_field("push_out", volume, field)
    if not field.signed or not field.cap:
        raise ValueError("push_out: the field must be signed and capped: volume.distance_field(signed=True, max_distance=...)")
    box, keep, step, _ = approach_volume.hand_lattice("push_out", volume, depth, width, B, params.step, None, x_extent)
    L = approach_volume.local_to_volume(grasp, to_volume)[3] if rows is None else rows[2]
    T = int(params.iterations)
    axes = np.ascontiguousarray(np.asarray(params.axes, dtype=np.float32))
    nx, ny, nz = p.dims
    pose = torch.empty((B, 12), dtype=torch.float32, device=dev)
    shift = torch.empty((B, 3), dtype=torch.float32, device=dev)
    trace = torch.empty((B, T + 1), dtype=torch.float32, device=dev)
    info = torch.empty((B, 4), dtype=torch.int32, device=dev)
    _lib.call("regnet_grasp_push_out_f32", field.dist2, field.dist2.data_ptr(), nx, ny, nz, volume.origin.ctypes.data, float(p.voxel),
              int(field.outside), L.data_ptr(), B, *box, step, x_extent, axes.ctypes.data, float(params.target),
              float(params.max_shift), T, pose.data_ptr(), shift.data_ptr(), trace.data_ptr(), info.data_ptr())
    return PushOut(pose, shift, info, trace, L, params)
