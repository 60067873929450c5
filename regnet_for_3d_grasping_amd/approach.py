"""Approach analysis on the device (csrc/approach.hip): what a robot needs in order to execute a collision-free grasp.

The collision filter (``eval_collision.no_collision_mask``) tests the hand at the final pose only and every grasp is reported at
the reference's fixed 8 cm opening.  ``analyse`` scans the cloud once more in every grasp's local frame and gives, per grasp,

* ``clearance``: the longest straight retreat along ``-approach`` from the final pose, capped at ``standoff``, on which the hand
  (palm and fingers, swept back) touches no point of the cloud -- a grasp behind which the neighbouring object stands has less
  than the standoff;
* ``width`` / ``offset`` / ``opening``: the extent of the object between the fingers along the closing axis, how far its middle
  sits off the gripper's centre line, and the opening to command (the extent plus a pad on either side, at most the gripper's);
* ``contact``: with ``friction_deg``, the share of the points in either contact band whose normal lies within the friction
  cone of the closing axis, left share times right share -- the antipodal test of the validation score
  (``eval_collision.antipodal_scores``) as counts on the observed cloud, without ground-truth normals and without a
  floating-point sum;
* ``pregrasp``: the point the gripper's centre starts its straight approach from, ``centre - approach * clearance``.

The arithmetic is pinned (include/regnet_hip.h, DESIGN.md par. 5): float32, every operation rounded on its own, integer counts
and min / max only, so ``tests/approach_reference.py`` restates it in numpy and the two agree exactly.  Nothing here reads from the
device or waits for it: ``analyse`` can be captured into a graph.  GPU only: there is no CPU path.
"""
import math
from dataclasses import dataclass, field as dataclass_field
from typing import Optional

import numpy as np
import torch

from . import _lib, eval_collision, grasp_select
from ._frame_util import ParamsBase, check_step, require_cuda, to_device

SPACES = ("cloud", "volume")        # what the hand is held against: ``analyse``'s points or ``analyse_volume``'s TSDF volume
UNSEEN = ("free", "blocked")        # what ``analyse_volume``'s clearance makes of space no camera has seen


@dataclass
class ApproachParams(ParamsBase):
    """What ``GraspDetector(approach=...)`` takes (a dict with these keys works too).  ``source``: the grasp set that is analysed
    (None: the ``select`` source, else ``"grasp_stage3"``); ``standoff``: how far back the approach is swept [m];
    ``contact_depth``: the depth of a contact band [m]; ``friction_deg``: the half angle of the friction cone -- None: no normals
    are estimated, the contact check does not run and ``contact`` is 0; ``normal_radius`` / ``normal_max_nn``: the neighbourhood
    ``eval_collision.estimate_normals`` fits a normal to; ``pad``: added to the measured width on either side for the opening
    [m]; ``min_clearance`` / ``min_contact``: None, or the least clearance [m] / contact share a grasp must have to be selected.

    The defaults are a choice made from the reference's gripper constants (6 cm palm-to-tip, 8 cm opening, the validation score's
    5 mm band and 1 cm / 30-neighbour normals).  Nobody has measured them on a robot.

    ``space``: ``"cloud"`` -- ``analyse``, the hand against the points -- or ``"volume"``: ``analyse_volume``, the hand against
    the detector's TSDF volume, which also knows what no camera has seen.  The other three are read in volume space only.
    ``unseen``: what ``clearance`` (and so ``pregrasp`` and ``min_clearance``) makes of space that is outside the volume or was
    never observed: ``"free"`` -- only seen surfaces block -- or ``"blocked"``.  ``step``: the distance between two samples of the
    swept hand [m]; None: the volume's voxel.  ``margin``: a voxel counts as solid when its distance to the surface is below
    this [m] (0: inside the surface), at most the volume's truncation distance to mean anything.  These defaults, too, are a
    choice nobody has measured on a robot.

    ``field``: in volume space, also build the volume's distance field (``tsdf.Volume.distance_field``) once per frame and read
    the hand against it: ``margin_hand`` / ``margin_sweep``, the distance [m] from the hand / the swept hand to the nearest
    obstacle -- solid voxels, and with ``unseen="blocked"`` unobserved voxels and the volume's outside too.  ``min_margin``:
    None, or the least ``margin_hand`` [m] a grasp must have to be selected; it needs ``field``.  (``margin`` above is the SOLID
    threshold, not this.)  ``field_signed``: build the field SIGNED (``distance_field(signed=True)``): a hand in collision reads a
    negative ``margin_hand``, minus the depth of its deepest sample, the record gains ``grasp_colliding``, and ``min_margin``
    judges the signed value: it may then be negative, e.g. -0.002 lets a hand through that is at most 2 mm inside an obstacle.  ``field_max_distance``: None, or ``distance_field``'s ``max_distance`` [m], the cap that bounds
    the field's cost; margins saturate there.  Both need ``field``.

    ``retreat``: None, True (the defaults) or a ``retreat.RetreatParams`` / a dict of its fields: also move the hand at its final
    pose along a fan of retreat directions and read the field at every step (``approach.retreat_fan``); the record gains the
    picked direction, its free length, margin and pre-grasp point.  ``min_retreat``: None, or the least free length [m] of the
    picked direction a grasp must have to be selected.  Both need ``space="volume"`` and ``field=True``; both are keyword-only.  Off by default (``retreat=False`` is None); the
    fan's defaults, too, are a choice nobody has measured on a robot."""
    WORD = "approach"
    source: Optional[str] = None
    standoff: float = 0.10
    contact_depth: float = eval_collision.NEIGHBOR_DEPTH
    friction_deg: Optional[float] = None
    normal_radius: float = eval_collision.NORMAL_RADIUS
    normal_max_nn: int = eval_collision.NORMAL_MAX_NN
    pad: float = 0.005
    min_clearance: Optional[float] = None
    min_contact: Optional[float] = None
    space: str = "cloud"
    unseen: str = "free"
    step: Optional[float] = None
    margin: float = 0.0
    field: bool = False
    min_margin: Optional[float] = None
    # keyword-only, so the positional order of the fields around them is what it was
    retreat: Optional[object] = dataclass_field(default=None, kw_only=True)
    min_retreat: Optional[float] = dataclass_field(default=None, kw_only=True)
    field_signed: bool = False
    field_max_distance: Optional[float] = None

    def __post_init__(self):
        if self.retreat is False:                 # off, as None is
            self.retreat = None
        if self.retreat is not None or self.min_retreat is not None:
            if self.space != "volume" or not self.field:
                raise ValueError("approach: retreat and min_retreat read the distance field of the TSDF volume; set "
                                 "space=\"volume\" and field=True")
            if self.retreat is None:
                raise ValueError("approach: min_retreat is judged on the retreat fan; set retreat=True (or its parameters)")
            if self.min_retreat is not None and not (float(self.min_retreat) >= 0.0 and np.isfinite(self.min_retreat)):
                raise ValueError("approach: min_retreat must be None or non-negative and finite")
            from . import retreat as retreat_mod
            self.retreat = retreat_mod.RetreatParams() if self.retreat is True else retreat_mod.RetreatParams.coerce(self.retreat)
            if float(self.retreat.min_margin) < 0.0 and not self.field_signed:
                raise ValueError("approach: a negative retreat min_margin is a tolerated penetration; it needs field_signed=True")
        if (self.field_signed or self.field_max_distance is not None) and not self.field:
            raise ValueError("approach: field_signed and field_max_distance shape the distance field; set field=True (and "
                             "space=\"volume\")")
        if self.field_max_distance is not None and not (float(self.field_max_distance) > 0.0
                                                        and np.isfinite(self.field_max_distance)):
            raise ValueError("approach: field_max_distance must be None or positive and finite")
        if self.field and self.space != "volume":
            raise ValueError("approach: field=True builds the distance field of the TSDF volume; use space=\"volume\" with it")
        if self.min_margin is not None:
            if not self.field:
                raise ValueError("approach: min_margin is judged on the distance field; set field=True (and space=\"volume\")")
            if not np.isfinite(self.min_margin) or (float(self.min_margin) < 0.0 and not self.field_signed):
                raise ValueError("approach: min_margin must be None or non-negative and finite (a signed field, field_signed=True, "
                                 "also takes a negative one: the penetration that is tolerated)")
        if self.space not in SPACES:
            raise ValueError("approach: space must be one of %s, not %r" % (", ".join(SPACES), self.space))
        if self.unseen not in UNSEEN:
            raise ValueError("approach: unseen must be one of %s, not %r" % (", ".join(UNSEEN), self.unseen))
        check_step("approach", self.step)
        if not (float(self.margin) >= 0.0 and np.isfinite(self.margin)):
            raise ValueError("approach: margin must be non-negative and finite")
        if self.source is not None and self.source not in grasp_select.SOURCES:
            raise ValueError("approach: source must be None or one of %s, not %r" % (", ".join(grasp_select.SOURCES), self.source))
        if not (float(self.standoff) >= 0.0 and np.isfinite(self.standoff)):
            raise ValueError("approach: standoff must be non-negative and finite")
        if not (float(self.contact_depth) >= 0.0 and float(self.pad) >= 0.0):
            raise ValueError("approach: contact_depth and pad must be non-negative")
        if self.friction_deg is not None and not 0.0 <= float(self.friction_deg) <= 90.0:
            raise ValueError("approach: friction_deg must be None or within [0, 90]")
        if not (float(self.normal_radius) > 0.0 and int(self.normal_max_nn) >= 3):
            raise ValueError("approach: normal_radius must be positive and normal_max_nn at least 3")

    # the hand paths are ``PathApproachParams``' fields; off here (class attributes, so that every reader may ask for them)
    paths = None
    min_path = None
    # ... and the push-out is ``PushApproachParams'``
    push = None
    push_keep = "all"

    @classmethod
    def coerce(cls, value):
        """``ParamsBase.coerce``; a dict that names ``paths`` or ``min_path`` becomes a ``PathApproachParams``, one that names
        ``push`` or ``push_keep`` a ``PushApproachParams`` (which has the paths' fields too)."""
        if cls is ApproachParams and isinstance(value, dict):
            if "push" in value or "push_keep" in value:
                return PushApproachParams(**value)
            if "paths" in value or "min_path" in value:
                return PathApproachParams(**value)
        return super().coerce(value)

    def filters(self):
        """Whether ``passes()`` can drop a grasp at all."""
        return (self.min_clearance is not None or self.min_contact is not None or self.min_margin is not None
                or self.min_retreat is not None or self.min_path is not None)


@dataclass
class PathApproachParams(ApproachParams):
    """``ApproachParams`` with the hand paths (``approach.check_paths``), both keyword-only.  ``paths``: None, True (the
    defaults) or a ``hand_path.PathParams`` / a dict of its fields: also take the hand through candidate trajectories of POSES --
    the fan's five directions and four turns of the straight retreat, or ``PathParams.paths`` -- and read the field at every
    waypoint; the record gains the picked path, every path's free and certified steps, the picked path's margin and the
    pre-grasp pose.  ``min_path``: None, or the least CERTIFIED length [m] of the picked path (``PathCheck.certified_length``) a
    grasp must have to be selected.  Both need ``space="volume"`` and ``field=True``.  Off by default (``paths=False`` is None);
    independent of ``retreat``.  A dict with either key handed to ``ApproachParams.coerce`` (``GraspDetector(approach=...)``,
    ``analyse_volume``) builds this class; ``ApproachParams``' own constructor is what it was.  The defaults of the paths, too, are
    a choice nobody has measured on a robot."""
    paths: Optional[object] = dataclass_field(default=None, kw_only=True)
    min_path: Optional[float] = dataclass_field(default=None, kw_only=True)

    def __post_init__(self):
        if self.paths is False:                   # off, as None is
            self.paths = None
        if self.paths is not None or self.min_path is not None:
            if self.space != "volume" or not self.field:
                raise ValueError("approach: paths and min_path read the distance field of the TSDF volume; set "
                                 "space=\"volume\" and field=True")
            if self.paths is None:
                raise ValueError("approach: min_path is judged on the hand paths; set paths=True (or their parameters)")
            if self.min_path is not None and not (float(self.min_path) >= 0.0 and np.isfinite(self.min_path)):
                raise ValueError("approach: min_path must be None or non-negative and finite")
            from . import hand_path
            self.paths = hand_path.PathParams() if self.paths is True else hand_path.PathParams.coerce(self.paths)
            if float(self.paths.min_margin) < 0.0 and not self.field_signed:
                raise ValueError("approach: a negative paths min_margin is a tolerated penetration; it needs field_signed=True")
        super().__post_init__()


PUSH_KEEP = ("all", "freed")       # what the selection sees of a pushed set: every grasp, or only those that have the target margin


@dataclass
class PushApproachParams(PathApproachParams):
    """``PathApproachParams`` with the push-out (``approach.push_out``), both keyword-only.  ``push``: None, True (the defaults)
    or a ``hand_adjust.PushParams`` / a dict of its fields: before anything else is analysed, move every hand that has less than
    the target margin along the signed field's gradient; a grasp the move FREED is analysed -- classification, margins, fan and
    paths -- at its moved centre, every other grasp as it was, and the record gains the status, the shift, the margin and the
    moved centre.  ``push_keep``: ``"all"``, or ``"freed"``: a grasp that does not have the target margin after the push-out
    (neither ALREADY_FREE nor FREED) is hidden from the selection.  Needs ``space="volume"``, ``field=True``,
    ``field_signed=True`` and a ``field_max_distance`` (the interpolation needs finite corners).  Off by default
    (``push=False`` is None).  A dict with either key handed to ``ApproachParams.coerce`` builds this class;
    ``ApproachParams'`` own constructor is what it was.  The defaults of the push-out, too, are a choice nobody has measured on
    a robot."""
    push: Optional[object] = dataclass_field(default=None, kw_only=True)
    push_keep: str = dataclass_field(default="all", kw_only=True)

    def __post_init__(self):
        if self.push is False:                    # off, as None is
            self.push = None
        if self.push_keep not in PUSH_KEEP:
            raise ValueError("approach: push_keep must be one of %s, not %r" % (", ".join(PUSH_KEEP), self.push_keep))
        if self.push is None and self.push_keep != "all":
            raise ValueError("approach: push_keep is judged on the push-out; set push=True (or its parameters)")
        if self.push is not None:
            if self.space != "volume" or not self.field or not self.field_signed or self.field_max_distance is None:
                raise ValueError("approach: push follows the gradient of the signed, capped distance field of the TSDF volume; set "
                                 "space=\"volume\", field=True, field_signed=True and a field_max_distance")
            from . import hand_adjust
            self.push = hand_adjust.PushParams() if self.push is True else hand_adjust.PushParams.coerce(self.push)
        super().__post_init__()

    def filters(self):
        return super().filters() or (self.push is not None and self.push_keep == "freed")


def cos_friction(friction_deg):
    """cos(friction angle) evaluated in float64 and rounded once to float32, as a Python float; None (no contact check) -> 0."""
    return 0.0 if friction_deg is None else float(np.float32(math.cos(math.radians(float(friction_deg)))))


class Approach:
    """``analyse``'s result, all on the device.  ``counts`` (B,8) int32 = (n_region, n_block, n_hand, n_left, ok_left, n_right,
    ok_right, 0) and ``values`` (B,4) float32 = (y_min, y_max, clearance, x_min) are the kernel's; ``frame`` (B,3,3) / ``center``
    (B,3) are ``eval_collision.grasp_frames``'.  The derived tensors are float32, one operation per step."""

    def __init__(self, counts, values, frame, center, params, half_space):
        self.counts, self.values, self.frame, self.center, self.params = counts, values, frame, center, params
        self.half_space = float(np.float32(half_space))

    @property
    def clearance(self):
        return self.values[:, 2]

    @property
    def empty(self):
        """(B) bool: nothing lies between the fingers."""
        return self.counts[:, 0] == 0

    @property
    def width(self):
        """y_max - y_min, 0 where the region is empty."""
        w = self.values[:, 1] - self.values[:, 0]
        return torch.where(self.empty, torch.zeros_like(w), w)

    @property
    def offset(self):
        """(y_max + y_min) * 0.5: the object's middle off the gripper's centre line, along axis_y; 0 where the region is empty."""
        o = (self.values[:, 1] + self.values[:, 0]) * 0.5
        return torch.where(self.empty, torch.zeros_like(o), o)

    @property
    def opening(self):
        """min(width + (pad + pad), hs + hs), the float32 constants formed first."""
        pad = np.float32(self.params.pad)
        hs = np.float32(self.half_space)
        return torch.clamp(self.width + float(np.float32(pad + pad)), max=float(np.float32(hs + hs)))

    @property
    def contact(self):
        """(ok_left / n_left) * (ok_right / n_right), 0 where either band is empty or the contact check did not run."""
        c = self.counts.to(torch.float32)
        share = (c[:, 4] / c[:, 3]) * (c[:, 6] / c[:, 5])
        return torch.where((self.counts[:, 3] == 0) | (self.counts[:, 5] == 0), torch.zeros_like(share), share)

    @property
    def pregrasp(self):
        """(B,3): centre - approach * clearance."""
        return self.center - self.frame[:, :, 0] * self.clearance.unsqueeze(1)

    def passes(self):
        """(B) bool: clearance >= min_clearance and contact >= min_contact, compared as float32; a bound that is None is not
        applied."""
        p = self.params
        ok = torch.ones((self.counts.shape[0],), dtype=torch.bool, device=self.counts.device)
        if p.min_clearance is not None:
            ok = ok & (self.clearance >= float(np.float32(p.min_clearance)))
        if p.min_contact is not None:
            ok = ok & (self.contact >= float(np.float32(p.min_contact)))
        return ok


def analyse(points, grasp, depth, width, params=None, normals=None):
    """``points`` (N,3) float32 on the GPU, any strides; ``grasp`` (B, >=8) float32 on the GPU; ``depth``: a float or one depth
    per grasp; ``width``: the gripper's opening (``eval_collision``'s box); ``params``: ``ApproachParams`` / a dict / None (the
    defaults); ``normals`` (N,3) float32 on the GPU, any strides, or None -- with ``friction_deg`` set they are then estimated
    (``eval_collision.estimate_normals``; the sign of a normal does not matter to |n_y|), without it the contact check does not
    run.  -> ``Approach``.  One launch on the current stream, no host read."""
    params = ApproachParams.coerce(params) or ApproachParams()
    require_cuda("points", points, torch.float32, 3, error=RuntimeError)
    require_cuda("grasp", grasp, torch.float32, 8, at_least=True, error=RuntimeError)
    dev = points.device
    N, B = int(points.shape[0]), int(grasp.shape[0])
    frame, center = eval_collision.grasp_frames(grasp[:, :8].contiguous())
    T = eval_collision.global_to_local(frame, center).contiguous()
    if not isinstance(depth, torch.Tensor) and np.ndim(depth) > 0:
        depth = to_device(np.asarray(depth, dtype=np.float32), dev)
    box, keep = eval_collision._box_args(depth, width, B, dev)
    if params.friction_deg is None:
        normals = None
    elif normals is None:
        normals = eval_collision.estimate_normals(points, radius=params.normal_radius, max_nn=params.normal_max_nn)
    if normals is not None:
        require_cuda("normals", normals, torch.float32, 3, error=RuntimeError)
        if normals.shape[0] != N or normals.device != dev:
            raise RuntimeError("normals must have one row per point, on the points' device")
    counts = torch.empty((B, 8), dtype=torch.int32, device=dev)
    values = torch.empty((B, 4), dtype=torch.float32, device=dev)
    n_args = (None, 0, 0) if normals is None else (normals.data_ptr(), normals.stride(0), normals.stride(1))
    _lib.call("regnet_grasp_approach_f32", points, points.data_ptr(), points.stride(0), points.stride(1), *n_args, N,
              T.data_ptr(), B, *box, float(params.standoff), float(params.contact_depth), cos_friction(params.friction_deg),
              counts.data_ptr(), values.data_ptr())
    return Approach(counts, values, frame, center, params, box[5])


def analyse_volume(volume, grasp, depth, width, params=None, to_volume=None, surface=None, max_depth=None, field=None):
    """The hand against a ``tsdf.Volume`` instead of a cloud: ``approach_volume.analyse_volume``, which is imported only here
    (and ``approach.VolumeApproach`` is its result's class)."""
    from . import approach_volume
    return approach_volume.analyse_volume(volume, grasp, depth, width, params, to_volume, surface, max_depth, field)


def retreat_fan(volume, field, grasp, depth, width, params=None, to_volume=None, max_depth=None):
    """Several retreat directions per grasp against the volume's distance field: ``retreat.retreat_fan``, which is imported only
    here (``approach.RetreatParams`` / ``approach.RetreatFan`` are its classes)."""
    from . import retreat
    return retreat.retreat_fan(volume, field, grasp, depth, width, params, to_volume, max_depth)


def check_paths(volume, field, grasp, depth, width, params=None, to_volume=None, max_depth=None, rows=None, poses=None):
    """Posed hand trajectories per grasp against the volume's distance field: ``hand_path.check_paths``, which is imported only
    here (``approach.PathParams`` / ``approach.PathCheck`` are its classes)."""
    from . import hand_path
    return hand_path.check_paths(volume, field, grasp, depth, width, params, to_volume, max_depth, rows, poses)


def push_out(volume, field, grasp, depth, width, params=None, to_volume=None, max_depth=None, rows=None):
    """Colliding hands moved free along the gradient of the volume's signed distance field: ``hand_adjust.push_out``, which is
    imported only here (``approach.PushParams`` / ``approach.PushOut`` are its classes)."""
    from . import hand_adjust
    return hand_adjust.push_out(volume, field, grasp, depth, width, params, to_volume, max_depth, rows)


def __getattr__(name):
    if name in ("PushParams", "PushOut"):
        from . import hand_adjust
        return getattr(hand_adjust, name)
    if name == "VolumeApproach":
        from . import approach_volume
        return approach_volume.VolumeApproach
    if name in ("PathParams", "PathCheck"):
        from . import hand_path
        return getattr(hand_path, name)
    if name in ("RetreatParams", "RetreatFan"):
        from . import retreat
        return getattr(retreat, name)
    raise AttributeError("module %r has no attribute %r" % (__name__, name))
