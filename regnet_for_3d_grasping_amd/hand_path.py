"""Hand paths (csrc/hand_path.hip): posed trajectories of the hand, checked against the volume's distance field.

The retreat fan (``retreat.retreat_fan``) translates the rigid hand at its final pose.  ``check_paths`` takes, per grasp, R
candidate paths of K + 1 POSES each -- waypoint 0 is the final grasp pose -- and reads the distance field under the hand's sample
lattice at every waypoint, so a path may turn the wrist as it backs out.  Per grasp and path it reports how many steps are free
and with what margin, picks the best path with the fan's pick kernel, and gives ``disp``, the largest distance any point of the
hand's bounding box moves between two waypoints: with it ``PathCheck.certified_steps`` says for which steps the sampled margins
also cover the motion between the samples (under a stated assumption).

``straight_paths`` / ``turn_paths`` / ``default_paths`` generate local paths on the host; a planner that has its own trajectories
hands them in as ``poses=``.  The arithmetic is pinned (include/regnet_hip.h "hand paths"), so ``tests/hand_path_reference.py``
restates it in numpy and the two agree exactly.  Nothing here reads from the device or waits for it.  GPU only: there is no CPU
path.
"""
import math
from dataclasses import dataclass
from typing import Any, Optional

import numpy as np
import torch

from . import _lib, approach_volume
from ._frame_util import ParamsBase, check_step, to_device
from .retreat import EDT_NONE, MAX_DIRECTIONS as MAX_PATHS, MAX_STEPS, StepCheck, threshold_word

__all__ = ["PathParams", "PathCheck", "straight_paths", "turn_paths", "default_paths", "compose", "check_paths"]


@dataclass
class PathParams(ParamsBase):
    """What ``check_paths`` takes (a dict with these keys works too).  ``length``: how far every generated path translates [m];
    ``steps``: K, the steps it is cut into (1..64); ``tilt_deg``: the tilt of the four side directions off the straight retreat,
    as in ``retreat.RetreatParams``; ``turn_deg``: the angle the four turning paths have turned through at their last waypoint
    (within [-180, 180]); ``pivot``: the point of the hand's LOCAL frame (x: approach, y: closing axis) the turns are about;
    ``paths``: explicit LOCAL paths, (R,K+1,12) shared by all grasps or (B,R,K+1,12), overriding the generated ones -- every
    waypoint the three rows of a pose of the hand relative to its final pose, waypoint 0 the identity; list them in order of
    preference, ties go to the first; ``min_margin``: a step is free when the hand's margin there is at least this [m] (a signed
    field also takes a negative value); ``step``: the distance between two samples of the hand [m]; None: the volume's voxel.

    The defaults -- a 10 cm path in 5 mm steps, a 25 degree fan, a 20 degree turn about the hand's origin -- are choices.  Nobody
    has measured them on a robot."""
    WORD = "paths"
    length: float = 0.10
    steps: int = 20
    tilt_deg: float = 25.0
    turn_deg: float = 20.0
    pivot: Any = (0.0, 0.0, 0.0)
    paths: Optional[Any] = None
    min_margin: float = 0.0
    step: Optional[float] = None

    def __post_init__(self):
        if not (float(self.length) >= 0.0 and np.isfinite(self.length)):
            raise ValueError("paths: length must be non-negative and finite")
        if int(self.steps) != self.steps or not 1 <= int(self.steps) <= MAX_STEPS:
            raise ValueError("paths: steps must be an integer in 1..%d" % MAX_STEPS)
        if not 0.0 <= float(self.tilt_deg) <= 90.0:
            raise ValueError("paths: tilt_deg must lie within [0, 90]")
        if not -180.0 <= float(self.turn_deg) <= 180.0:
            raise ValueError("paths: turn_deg must lie within [-180, 180]")
        pivot = np.asarray(self.pivot, dtype=np.float64)
        if pivot.shape != (3,) or not np.isfinite(pivot).all():
            raise ValueError("paths: pivot must be a finite 3-vector")
        if self.paths is not None:
            shape = tuple(self.paths.shape) if hasattr(self.paths, "shape") else np.shape(self.paths)
            if len(shape) not in (3, 4) or shape[-1] != 12 or not 2 <= shape[-2] <= MAX_STEPS + 1 or not 1 <= shape[-3] <= MAX_PATHS:
                raise ValueError("paths: paths must be (R,K+1,12) or (B,R,K+1,12) with R in 1..%d and K in 1..%d" % (MAX_PATHS, MAX_STEPS))
        if not np.isfinite(self.min_margin):
            raise ValueError("paths: min_margin must be finite")
        check_step("paths", self.step)


def _rotation(axis, angle):
    """Rodrigues' rotation about the unit float64 ``axis``: I + sin K + (1 - cos) K K; the identity exactly at angle 0."""
    x, y, z = axis
    K = np.array([[0.0, -z, y], [z, 0.0, -x], [-y, x, 0.0]])
    return np.eye(3) + (math.sin(angle) * K + (1.0 - math.cos(angle)) * (K @ K))


def turn_paths(dirs, axis, pivot, angle_deg, length, K):
    """-> (R, K+1, 12) float32 LOCAL poses, built on the host in float64 and rounded once: waypoint k of row r is
    ``Trans(k ds d_r) . Rot(axis, k angle / K, about pivot)`` with ``ds = length / K`` -- the hand turns about ``pivot`` by an
    angle that grows linearly to ``angle_deg`` while it translates along ``d_r``, used as given (not normalised).  ``axis`` is
    normalised.  Waypoint 0 is the identity exactly."""
    dirs = np.asarray(dirs, dtype=np.float64).reshape(-1, 3)
    axis = np.asarray(axis, dtype=np.float64).reshape(3)
    pivot = np.asarray(pivot, dtype=np.float64).reshape(3)
    K = int(K)
    if not 1 <= K <= MAX_STEPS:
        raise ValueError("paths: K must be in 1..%d" % MAX_STEPS)
    norm = float(np.linalg.norm(axis))
    if not (norm > 0.0 and np.isfinite(norm)):
        raise ValueError("paths: the turn's axis must be a finite, non-zero 3-vector")
    axis = axis / norm
    ds, angle = float(length) / K, math.radians(float(angle_deg))
    out = np.zeros((dirs.shape[0], K + 1, 3, 4), dtype=np.float64)
    for k in range(K + 1):
        rot = _rotation(axis, k * angle / K)
        out[:, k, :, :3] = rot
        out[:, k, :, 3] = (pivot - rot @ pivot)[None, :] + (k * ds) * dirs
    return out.reshape(dirs.shape[0], K + 1, 12).astype(np.float32)


def straight_paths(dirs, length, K):
    """-> (R, K+1, 12) float32: translation-only paths, waypoint k of row r the identity moved by ``k (length / K) d_r``."""
    return turn_paths(dirs, (0.0, 0.0, 1.0), (0.0, 0.0, 0.0), 0.0, length, K)


def default_paths(params=None):
    """The R = 9 default paths as (9, K+1, 12) float32 LOCAL poses: the five directions of ``retreat.default_fan`` as straight
    paths, in the fan's order (straight first, so a tie still prefers it); then the straight retreat turning by ``+turn_deg`` and
    ``-turn_deg`` about local z; then the same two about local y, all about ``pivot``."""
    params = PathParams.coerce(params) or PathParams()
    c, s = math.cos(math.radians(float(params.tilt_deg))), math.sin(math.radians(float(params.tilt_deg)))
    fan = [[-1.0, 0.0, 0.0], [-c, 0.0, s], [-c, 0.0, -s], [-c, s, 0.0], [-c, -s, 0.0]]
    K, length, turn = int(params.steps), float(params.length), float(params.turn_deg)
    rows = [straight_paths(fan, length, K)]
    for axis in ((0.0, 0.0, 1.0), (0.0, 1.0, 0.0)):
        for angle in (turn, -turn):
            rows.append(turn_paths(fan[:1], axis, params.pivot, angle, length, K))
    return np.concatenate(rows, axis=0)


def compose(L, local):
    """``L`` (B,12) float32 on the device, the grasps' local-to-volume rows; ``local`` (R,K+1,12) or (B,R,K+1,12) float32 local
    poses (a host array or a tensor) -> ``P`` (B,R,K+1,12) float32: every local pose times the grasp's ``L``, on the device in
    float64 and rounded once.  Entry (i, j) is ``(L[i,0] m[0,j] + L[i,1] m[1,j]) + L[i,2] m[2,j]``, and ``+ L[i,3]`` in the last
    column (a pose's fourth row is 0 0 0 1)."""
    dev = L.device
    B = int(L.shape[0])
    if not isinstance(local, torch.Tensor):
        local = to_device(np.ascontiguousarray(local, dtype=np.float32), dev)
    local = local.to(dev, torch.float64)
    if local.dim() == 3:
        local = local.unsqueeze(0)
    elif int(local.shape[0]) != B:
        raise ValueError("paths: per-grasp paths must be (B,R,K+1,12) with B = %d grasps" % B)
    R, K1 = int(local.shape[1]), int(local.shape[2])
    m = local.reshape(local.shape[0], R, K1, 3, 4)
    A = L.to(torch.float64).reshape(B, 1, 1, 3, 4)
    out = (A[..., :, 0:1] * m[..., 0:1, :] + A[..., :, 1:2] * m[..., 1:2, :]) + A[..., :, 2:3] * m[..., 2:3, :]
    out = torch.cat([out[..., :3], out[..., 3:] + A[..., 3:]], dim=-1)
    return out.reshape(B, R, K1, 12).to(torch.float32).contiguous()


class PathCheck(StepCheck):
    """``check_paths``' result, all on the device.  ``result`` (B,R,4) int32 = (free_steps, the minimum word over steps
    1..free_steps, the minimum over steps 1..K, OUTSIDE lookups over steps 1..K), ``profile`` (B,R,K+1) int32 and ``disp``
    (B,R,K) float32 are the check kernel's, ``best`` (B,4) int32 = (r*, its free_steps, its free-prefix minimum, 0) the fan's
    pick kernel's; ``P`` (B,R,K+1,12) float32 the poses that were checked, ``thresh`` the word ``min_margin`` became, ``step``
    the lattice step [m].  ``free_steps``, ``profile_metres``, ``index`` and ``margin`` are ``StepCheck``'s."""

    def __init__(self, result, profile, best, disp, P, field, thresh, step, voxel, params):
        self.result, self.profile, self.best, self.disp, self.P = result, profile, best, disp, P
        self.field, self.thresh, self.step, self.voxel, self.params = field, int(thresh), float(step), float(voxel), params

    def length_at(self, steps):
        """``steps`` (B) integers in 0..K -> (B) float32 [m]: how far the hand's farthest point moves on the PICKED path up to
        that step, ``disp[0] + disp[1] + ...`` of the path's first ``steps`` entries, summed in float32 from the left by K
        elementwise additions (a fixed order: the same bytes on every run; no host read)."""
        B, K = int(self.disp.shape[0]), int(self.disp.shape[2])
        row = torch.gather(self.disp, 1, self.index.view(B, 1, 1).expand(B, 1, K)).reshape(B, K)
        steps = steps.to(torch.int64)
        total = torch.zeros((B,), dtype=torch.float32, device=self.disp.device)
        for k in range(K):
            total = torch.where(steps > k, total + row[:, k], total)
        return total

    @property
    def free_length(self):
        """(B) float32 [m]: ``length_at`` the picked path's last free step."""
        return self.length_at(self.best[:, 1])

    @property
    def waypoint(self):
        """(B,12) float32: the picked path's pose at its last free step, as the three rows of the hand's local-to-volume
        matrix -- the pre-grasp POSE the hand starts its way in from (the final pose itself where no step is free)."""
        B, K1 = int(self.best.shape[0]), int(self.P.shape[2])
        flat = self.index * K1 + self.best[:, 1].to(torch.int64)
        return torch.gather(self.P.reshape(B, -1, 12), 1, flat.view(B, 1, 1).expand(B, 1, 12)).reshape(B, 12)

    def default_slack(self):
        """``(step + voxel) * sqrt(3) / 2`` [m], in float64: a hand point is within half a lattice diagonal of a sample, and a
        sample within half a voxel diagonal of its voxel's centre."""
        return (self.step + self.voxel) * math.sqrt(3.0) / 2.0

    def certified_steps(self, slack=None):
        """(B,R) int32: the prefix of steps k = 1.. for which, in float32 elementwise operations,
        ``(min(metres[k-1], metres[k]) - disp[k-1] / 2) - slack >= min_margin`` -- the steps on which the margins sampled at the
        two waypoints also bound the margin of every point of the hand DURING the motion between them.  ``slack``: None is
        ``default_slack()``, what the lattice and the nearest-voxel lookup can hide.

        The assumption: between two waypoints every point of the hand moves on the CHORD between its two posed positions, so it
        stays within ``disp / 2`` of one of the two ends, where the field was sampled.  A robot that interpolates the two poses
        as a screw motion moves the point on an arc instead; the arc leaves the chord by its sagitta, ``r (1 - cos(a / 2))`` for
        a turn by ``a`` at distance ``r`` from the axis, which is second order in the step angle (0.02 mm for the default turn
        of 1 degree a step at 10 cm).  That term is NOT covered here: give it as extra ``slack`` where it matters.  A NaN
        anywhere certifies nothing from that step on."""
        slack = self.default_slack() if slack is None else float(slack)
        metres = self.profile_metres
        low = torch.minimum(metres[:, :, :-1], metres[:, :, 1:])
        room = (low - self.disp / 2.0) - float(np.float32(slack))
        ok = room >= float(np.float32(self.params.min_margin))
        return torch.cumprod(ok.to(torch.int32), dim=2).sum(dim=2).to(torch.int32)

    @property
    def certified_length(self):
        """(B) float32 [m]: ``length_at`` the picked path's last certified step (default slack) -- what
        ``PathApproachParams.min_path`` judges."""
        B = int(self.best.shape[0])
        return self.length_at(torch.gather(self.certified_steps(), 1, self.index.view(B, 1)).reshape(B))

    def passes(self, minimum):
        """(B) bool for the picked path.  An ``int`` is a number of steps: ``free_steps >= minimum``.  A ``float`` is a length
        [m]: ``free_length >= minimum``, compared as float32."""
        if isinstance(minimum, (int, np.integer)) and not isinstance(minimum, bool):
            return self.best[:, 1] >= int(minimum)
        return self.free_length >= float(np.float32(minimum))


def check_paths(volume, field, grasp, depth, width, params=None, to_volume=None, max_depth=None, rows=None, poses=None):
    """``volume``, ``field``, ``grasp``, ``depth``, ``width``, ``to_volume``, ``max_depth`` and ``rows`` as in
    ``retreat.retreat_fan``; ``params``: ``PathParams`` / a dict / None (the defaults).  -> ``PathCheck``.

    ``poses``: the planner's use -- (B,R,K+1,12) or (B,R,K+1,4,4) float32 on the device, the hand's local-to-volume pose at
    every waypoint, ALREADY in the volume's frame and used as given (``to_volume`` does not touch them); waypoint 0 is the final
    grasp pose.  Without ``poses`` they are ``compose(L, params.paths or default_paths(params))``.

    A step is FREE as in the fan: the minimum field word over the hand's samples at the waypoint is ``>= thresh``, the smallest
    word whose ``field.metres()`` value is ``>= float32(min_margin)`` (``retreat.threshold_word``).  No host read: capturable.
    Two launches on the current stream (the check, the fan's pick) when ``poses`` is a contiguous (B,R,K+1,12) tensor; a
    (B,R,K+1,4,4) or non-contiguous one is first copied to that layout (one torch copy more; only rows 0..2 are read and the
    fourth row is not checked), and without ``poses`` ``compose`` adds its torch operations."""
    params = PathParams.coerce(params) or PathParams()
    p = volume.params
    dev, B, depth, x_extent = approach_volume.hand_call("check_paths", volume, grasp, depth, max_depth)
    approach_volume.require_field("check_paths", volume, field)
    if float(params.min_margin) < 0.0 and not field.signed:
        raise ValueError("check_paths: a negative min_margin is a tolerated penetration; it needs a signed field")
    box, keep, step, _ = approach_volume.hand_lattice("check_paths", volume, depth, width, B, params.step, None, x_extent)
    if poses is not None:
        if not isinstance(poses, torch.Tensor) or poses.device != dev or poses.dtype != torch.float32:
            raise RuntimeError("check_paths: poses must be a float32 tensor on the volume's device")
        if poses.dim() == 5 and tuple(poses.shape[3:]) == (4, 4):
            poses = poses[:, :, :, :3, :].reshape(poses.shape[0], poses.shape[1], poses.shape[2], 12)
        if poses.dim() != 4 or int(poses.shape[0]) != B or int(poses.shape[3]) != 12:
            raise ValueError("check_paths: poses must be (B,R,K+1,12) or (B,R,K+1,4,4) with B = %d grasps" % B)
        P = poses.contiguous()
    else:
        L = approach_volume.local_to_volume(grasp, to_volume)[3] if rows is None else rows[2]
        P = compose(L, default_paths(params) if params.paths is None else params.paths)
    R, K = int(P.shape[1]), int(P.shape[2]) - 1
    if not (1 <= R <= MAX_PATHS and 1 <= K <= MAX_STEPS):
        raise ValueError("check_paths: %d paths of %d steps; at most %d paths and 1..%d steps" % (R, K, MAX_PATHS, MAX_STEPS))
    thresh = threshold_word(params.min_margin, p.voxel, field.signed)
    nx, ny, nz = p.dims
    profile = torch.empty((B, R, K + 1), dtype=torch.int32, device=dev)
    result = torch.empty((B, R, 4), dtype=torch.int32, device=dev)
    disp = torch.empty((B, R, K), dtype=torch.float32, device=dev)
    best = torch.empty((B, 4), dtype=torch.int32, device=dev)
    entry = "regnet_grasp_path_check_signed_f32" if field.signed else "regnet_grasp_path_check_f32"
    _lib.call(entry, field.dist2, field.dist2.data_ptr(), nx, ny, nz, volume.origin.ctypes.data, float(p.voxel), int(field.outside),
              P.data_ptr(), B, R, K, *box, step, x_extent, thresh, profile.data_ptr(), result.data_ptr(), disp.data_ptr())
    _lib.call("regnet_grasp_retreat_pick", result, result.data_ptr(), B, R, best.data_ptr())
    return PathCheck(result, profile, best, disp, P, field, thresh, step, p.voxel, params)
