"""Retreat fan (csrc/retreat.hip): several retreat directions per grasp, judged against the volume's distance field.

``approach.analyse_volume`` knows one motion, the straight sweep along ``-approach``; a grasp whose straight retreat is blocked by
a second object behind the hand, or by the unseen space behind an occluder, is dropped by ``min_clearance``.  ``retreat_fan``
moves the rigid hand at its final pose along a small fan of candidate directions -- straight, tilted to either side, tilted up
or down, and with ``up`` lifted -- in ``steps`` steps of ``length / steps`` and reads the distance field
(``tsdf.Volume.distance_field``) at every step.  Per grasp and direction it reports how many steps are free and with what
margin, picks the best direction and gives the pre-grasp point that goes with it.

The hand translates only: it does not rotate along the path.  Every value is a nearest-voxel lookup of a lattice sample,
quantised to the lattice step and to ``ds``.  The arithmetic is pinned (include/regnet_hip.h "retreat fan"), so
``tests/retreat_reference.py`` restates it in numpy and the two agree exactly.  Nothing here reads from the device or waits for
it.  GPU only: there is no CPU path.
"""
import math
from dataclasses import dataclass
from typing import Any, Optional

import numpy as np
import torch

from . import _lib, approach_volume
from ._frame_util import ParamsBase, check_step, to_device

EDT_NONE = 1 << 30
MAX_DIRECTIONS = 16                 # regnet_grasp_retreat_fan_f32's documented limits
MAX_STEPS = 64
MAX_WORD = 3 * 1023 * 1023          # the largest squared distance of a field whose dims are at most 1024


@dataclass
class RetreatParams(ParamsBase):
    """What ``retreat_fan`` and ``ApproachParams(retreat=...)`` take (a dict with these keys works too).  ``length``: the length
    of every candidate path [m]; ``steps``: K, the steps it is cut into (1..64), ``ds = length / steps``; ``tilt_deg``: the tilt
    of the fan's four side directions off the straight retreat; ``up``: None, or a 3-vector in the grasps' frame (the camera
    side, or against gravity) -- two per-grasp directions more: ``up`` itself in each grasp's local frame and the bisector of it
    and the straight retreat; ``directions``: an explicit (R,3) array shared by all grasps or a (B,R,3) one, in the grasps' LOCAL
    frames (x: approach, y: closing axis), used as given -- not normalised -- and overriding the fan; list them in order of
    preference, ties go to the first; ``min_margin``: a step is free when the hand's margin there is at least this [m] (a signed
    field also takes a negative value: the penetration that is tolerated); ``step``: the distance between two samples of the
    hand [m]; None: the volume's voxel.

    The defaults -- a 10 cm path in 5 mm steps, a 25 degree fan -- are a choice made from the reference's gripper constants and the
    approach analysis' standoff.  Nobody has measured them on a robot."""
    WORD = "retreat"
    length: float = 0.10
    steps: int = 20
    tilt_deg: float = 25.0
    up: Optional[Any] = None
    directions: Optional[Any] = None
    min_margin: float = 0.0
    step: Optional[float] = None

    def __post_init__(self):
        if not (float(self.length) >= 0.0 and np.isfinite(self.length)):
            raise ValueError("retreat: length must be non-negative and finite")
        if int(self.steps) != self.steps or not 1 <= int(self.steps) <= MAX_STEPS:
            raise ValueError("retreat: steps must be an integer in 1..%d" % MAX_STEPS)
        if not 0.0 <= float(self.tilt_deg) <= 90.0:
            raise ValueError("retreat: tilt_deg must lie within [0, 90]")
        if self.up is not None and not isinstance(self.up, torch.Tensor):
            up = np.asarray(self.up, dtype=np.float64)
            if up.shape != (3,) or not np.isfinite(up).all() or not np.linalg.norm(up) > 0.0:
                raise ValueError("retreat: up must be None or a finite, non-zero 3-vector")
        if self.directions is not None:
            shape = tuple(self.directions.shape) if hasattr(self.directions, "shape") else np.shape(self.directions)
            if len(shape) not in (2, 3) or shape[-1] != 3 or not 1 <= shape[-2] <= MAX_DIRECTIONS:
                raise ValueError("retreat: directions must be (R,3) or (B,R,3) with R in 1..%d" % MAX_DIRECTIONS)
        if not np.isfinite(self.min_margin):
            raise ValueError("retreat: min_margin must be finite")
        check_step("retreat", self.step)


def word_metres(word, voxel, signed):
    """The metres of ONE field word on the host, by ``DistanceField.metres``' float32 operations: unsigned
    ``sqrtf((float)w) * voxel_f``, signed ``copysignf((sqrtf((float)|s|) - 0.5f) * voxel_f, (float)s)``; +-inf for +-EDT_NONE."""
    word = int(word)
    if abs(word) >= EDT_NONE:
        return np.float32(-np.inf if word < 0 else np.inf)
    root = np.sqrt(np.float32(abs(word)))
    if not signed:
        return np.float32(root * np.float32(voxel))
    return np.float32(np.copysign(np.float32(np.float32(root - np.float32(0.5)) * np.float32(voxel)), np.float32(word)))


def threshold_word(min_margin, voxel, signed):
    """``thresh``: the SMALLEST field word whose ``metres()`` value is ``>= float32(min_margin)``, so that ``word >= thresh`` on
    the device is ``metres(word) >= min_margin`` exactly (the conversion is monotone in the word).  The words of an unsigned field
    are 0 .. 3 * 1023^2 and EDT_NONE (+inf); those of a signed field -3 * 1023^2 .. -1, 1 .. 3 * 1023^2 and +-EDT_NONE -- 0 is not
    a signed word and is never returned for one.  A bound that no finite word reaches gives EDT_NONE: only "no obstacle at all"
    is free then.  A bound at or below every finite word's value gives the lowest finite word, 0 or -3 * 1023^2: every step over
    finite words is free.  -EDT_NONE, the word of a signed field in which NO voxel is free, converts to -inf, which is below any
    finite bound: such a voxel is never free, however negative ``min_margin`` is (it is returned only for a bound of -inf,
    which ``RetreatParams`` does not accept)."""
    bound = np.float32(min_margin)
    lowest = -EDT_NONE if signed else 0
    if word_metres(lowest, voxel, signed) >= bound:
        return lowest
    lo, hi = (-MAX_WORD if signed else 0), MAX_WORD
    if not word_metres(hi, voxel, signed) >= bound:
        return EDT_NONE
    if word_metres(lo, voxel, signed) >= bound:
        return lo
    while hi - lo > 1:                                # metres(lo) < bound <= metres(hi)
        mid = (lo + hi) // 2
        if word_metres(mid, voxel, signed) >= bound:
            hi = mid
        else:
            lo = mid
    return 1 if (signed and hi == 0) else hi          # (0 converts like +1 and is not a word of a signed field)


def default_fan(tilt_deg, device, frame=None, up=None):
    """The default fan as unit float32 rows in LOCAL frames, on the device: straight (-1, 0, 0); (-cos, 0, +-sin) (tilted across
    the hand's thickness); (-cos, +-sin, 0) (tilted along the closing axis) -> (5,3), one table for all grasps.  With ``up`` (a
    3-vector in the grasps' frame) and ``frame`` (B,3,3): two per-grasp rows more -- ``frame^T up`` normalised, and the normalised
    bisector of it and straight (straight itself where the two cancel) -> (B,7,3).  Straight first: the pick prefers it on a tie."""
    c, s = math.cos(math.radians(float(tilt_deg))), math.sin(math.radians(float(tilt_deg)))
    table = to_device(np.array([[-1.0, 0.0, 0.0], [-c, 0.0, s], [-c, 0.0, -s], [-c, s, 0.0], [-c, -s, 0.0]], dtype=np.float32), device)
    if up is None:
        return table
    if not isinstance(up, torch.Tensor):
        up = to_device(np.asarray(up, dtype=np.float32).reshape(3), device)
    up = up.to(torch.float32).reshape(1, 3, 1)
    B = int(frame.shape[0])
    local = (frame.to(torch.float32).transpose(1, 2) @ up).reshape(B, 3)
    local = local / local.norm(dim=1, keepdim=True)
    mid = local + table[0]
    length = mid.norm(dim=1, keepdim=True)
    mid = torch.where(length > 1e-6, mid / length, table[0].expand(B, 3))
    return torch.cat([table.unsqueeze(0).expand(B, 5, 3), local.unsqueeze(1), mid.unsqueeze(1)], dim=1).contiguous()


class StepCheck:
    """What ``RetreatFan`` and ``hand_path.PathCheck`` share: R candidates per grasp (directions of the fan, paths) of K steps
    each, read off ``result`` (B,R,4) int32, ``profile`` (B,R,K+1) int32, ``best`` (B,4) int32 and the ``field`` they were
    checked against."""

    @property
    def free_steps(self):
        """(B,R) int32: per candidate the steps from the final pose on which the hand keeps ``min_margin``."""
        return self.result[:, :, 0]

    @property
    def profile_metres(self):
        """(B,R,K+1) float32 [m]: the hand's margin at every step, ``field.metres`` of ``profile``."""
        return self.field.metres(self.profile.contiguous())

    @property
    def index(self):
        """(B) int64: the picked candidate's row."""
        return self.best[:, 0].to(torch.int64)

    @property
    def margin(self):
        """(B) float32 [m]: the smallest margin over the picked candidate's free steps, +inf where it has none."""
        return self.field.metres(self.best[:, 2].contiguous())


class RetreatFan(StepCheck):
    """``retreat_fan``'s result, all on the device.  ``result`` (B,R,4) int32 = (free_steps, the minimum word over steps
    1..free_steps, the minimum over steps 1..K, OUTSIDE lookups over steps 1..K), ``profile`` (B,R,K+1) int32 and ``best`` (B,4)
    int32 = (r*, its free_steps, its free-prefix minimum, 0) are the kernels'; ``dirs`` (R,3) or (B,R,3) float32 the local
    directions they were given, ``L`` (B,12) the local-to-volume rows, ``thresh`` the word ``min_margin`` became, ``ds`` the step
    length [m].  ``index`` (``StepCheck``'s) is the picked direction's row in ``dirs``."""

    def __init__(self, result, profile, best, dirs, L, frame, center, field, thresh, ds, params):
        self.result, self.profile, self.best, self.dirs, self.L = result, profile, best, dirs, L
        self.frame, self.center, self.field, self.thresh, self.ds, self.params = frame, center, field, int(thresh), float(ds), params

    @property
    def free_length(self):
        """(B) float32 [m]: ``free_steps * ds`` of the picked direction."""
        return self.best[:, 1].to(torch.float32) * float(np.float32(self.ds))

    @property
    def direction(self):
        """(B,3) float32: the picked direction in the grasps' frame, ``frame @ d`` (torch, not bit-pinned)."""
        B = int(self.best.shape[0])
        table = self.dirs if self.dirs.dim() == 3 else self.dirs.unsqueeze(0).expand(B, -1, -1)
        local = torch.gather(table, 1, self.index.view(B, 1, 1).expand(B, 1, 3)).reshape(B, 3, 1)
        return (self.frame.to(torch.float32) @ local).reshape(B, 3)

    @property
    def pregrasp(self):
        """(B,3) float32: ``centre + direction * free_length``, where the hand starts its way in along the picked direction."""
        return self.center + self.direction * self.free_length.unsqueeze(1)

    def passes(self, min_retreat):
        """(B) bool: ``free_length >= min_retreat``, compared as float32."""
        return self.free_length >= float(np.float32(min_retreat))


def retreat_fan(volume, field, grasp, depth, width, params=None, to_volume=None, max_depth=None, rows=None):
    """``volume``: a ``tsdf.Volume``; ``field``: a ``tsdf.DistanceField`` of it (``volume.distance_field(...)``), signed or not;
    ``grasp`` (B, >=8) float32 on its device; ``depth``, ``width``, ``to_volume`` and ``max_depth`` as in
    ``approach.analyse_volume``, whose local-to-volume rows ``L`` these are (one function forms both); ``params``:
    ``RetreatParams`` / a dict / None (the defaults).  -> ``RetreatFan``.  Two launches on the current stream (the fan, the pick),
    no host read.

    A step of a direction is FREE when the minimum field word over the hand's samples there is ``>= thresh``, and ``thresh`` is
    derived on the host (``threshold_word``): the smallest word whose ``field.metres()`` value is ``>= float32(min_margin)`` --
    the conversion is monotone, so the integer test on the device is the metric one exactly.  For an unsigned field and the
    default ``min_margin = 0`` that is word 0: every step is free, obstacles included, so give a positive ``min_margin`` (half a
    voxel, say) or a signed field, whose default threshold is word 1, "not inside an obstacle".

    ``rows``: ``approach_volume.local_to_volume``'s ``(frame, center, L)`` of these grasps and this ``to_volume``, when the
    caller has formed them already (``analyse_volume`` has); None: they are formed here."""
    params = RetreatParams.coerce(params) or RetreatParams()
    p = volume.params
    dev, B, depth, x_extent = approach_volume.hand_call("retreat_fan", volume, grasp, depth, max_depth)
    approach_volume.require_field("retreat_fan", volume, field)
    if float(params.min_margin) < 0.0 and not field.signed:
        raise ValueError("retreat_fan: a negative min_margin is a tolerated penetration; it needs a signed field")
    frame, center, L = approach_volume.local_to_volume(grasp, to_volume)[1:] if rows is None else rows
    box, keep, step, _ = approach_volume.hand_lattice("retreat_fan", volume, depth, width, B, params.step, None, x_extent)
    if params.directions is not None:
        dirs = params.directions
        if not isinstance(dirs, torch.Tensor):
            dirs = np.asarray(dirs, dtype=np.float32)
        dirs = to_device(dirs, dev).to(torch.float32).contiguous()
        if dirs.dim() == 3 and int(dirs.shape[0]) != B:
            raise ValueError("retreat_fan: per-grasp directions must be (B,R,3) with B = %d grasps" % B)
    else:
        dirs = default_fan(params.tilt_deg, dev, frame, params.up)
    R, K = int(dirs.shape[-2]), int(params.steps)
    ds = float(params.length) / K
    thresh = threshold_word(params.min_margin, p.voxel, field.signed)
    nx, ny, nz = p.dims
    profile = torch.empty((B, R, K + 1), dtype=torch.int32, device=dev)
    result = torch.empty((B, R, 4), dtype=torch.int32, device=dev)
    best = torch.empty((B, 4), dtype=torch.int32, device=dev)
    entry = "regnet_grasp_retreat_fan_signed_f32" if field.signed else "regnet_grasp_retreat_fan_f32"
    _lib.call(entry, field.dist2, field.dist2.data_ptr(), nx, ny, nz, volume.origin.ctypes.data, float(p.voxel), int(field.outside),
              L.data_ptr(), B, *box, step, x_extent, dirs.data_ptr(), 3 * R if dirs.dim() == 3 else 0, R, K, ds, thresh,
              profile.data_ptr(), result.data_ptr())
    _lib.call("regnet_grasp_retreat_pick", result, result.data_ptr(), B, R, best.data_ptr())
    return RetreatFan(result, profile, best, dirs, L, frame, center, field, thresh, ds, params)
