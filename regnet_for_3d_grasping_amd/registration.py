"""Pose refinement on the device (csrc/icp.hip): point-to-plane ICP of a source cloud onto a target cloud.

``icp`` corrects the pose that takes ``source`` into ``target``'s frame: for every source row the nearest target row within
``max_dist`` (over the uniform grid of the target), the point-to-plane residual against that row's normal, the 6x6 normal
equations summed in a fixed order in float64, a Cholesky solve and the pose update -- two launches per iteration, the pose, the
status word and the per-iteration history in one small device block.  A step whose block is no longer RUNNING returns at once,
so the fixed number of steps is enqueued without reading anything back.  The arithmetic is pinned (include/regnet_hip.h,
DESIGN.md par. 5) and ``tests/icp_reference.py`` restates it in numpy: the correspondences agree exactly, the sums to float64
rounding.  ``fusion.refine_poses`` registers the views of several cameras onto one of them before ``fusion.voxel_merge``.

``association="projective"`` is a second way to find the pairs, for a target that is the organised cloud of a depth image
(``depth_frame.to_cloud``) in ITS camera's frame: a source row is taken into that frame, projected into the target's image and
paired with the nearest of the pixels in a small window around the one it falls on -- a lookup instead of a search over a grid,
as depth-camera pipelines (KinectFusion and its descendants) register frames.  The normals come from the image as well
(``depth_frame.normals``), nothing is compacted and nothing is read, and ``normal_angle`` additionally refuses a pair whose two
normals disagree, so that points only one camera sees do not pull the pose.  ``tests/icp_projective_reference.py`` restates it.
The grid search stays the tool for clouds without a pixel grid, and the default.

The host reads: the count of the target's finite rows while it is prepared (``prepare_target``, and ``prepare_projective_target``
with ``normals="fit"``), and the state block in ``Registration.result()``.
Nothing draws from numpy's random stream.  GPU only: there is no CPU path.
"""
from dataclasses import dataclass

import math
from typing import Optional

import numpy as np
import torch

from . import _lib
from ._frame_util import MAX_FRAME_POINTS, ParamsBase, matrix4, record_streams, require_cuda, stream_scope, to_device

_L = _lib.lib

RUNNING, CONVERGED, MAX_ITER, TOO_FEW, DEGENERATE = range(5)
STATUS_NAMES = ("RUNNING", "CONVERGED", "MAX_ITER", "TOO_FEW", "DEGENERATE")
MAX_ITERATIONS = 64                  # rows of the state block's history
STATE_BYTES = 128 + 16 * MAX_ITERATIONS
MAX_POINTS = MAX_FRAME_POINTS        # regnet_icp_*'s documented limit


@dataclass(frozen=True)
class IcpParams(ParamsBase):
    """``max_dist``: a source point pairs with its nearest target point when that is this close [m]; ``iterations``: the steps
    enqueued, 1..64; ``stride``: every so-manieth source row takes part -- the cloud of a depth image is organised row by row, so
    a stride that divides the image width visits whole pixel columns and nothing between them (4 on a 640-wide frame: every
    fourth column), which leaves the faces that hold the pose along a plane hardly sampled: take one that does not (3, 7, 9);
    ``min_pairs``: fewer pairs end the registration as
    TOO_FEW; ``rot_eps`` [rad] / ``trans_eps`` [m]: a step that turns and moves by less has CONVERGED; ``normal_radius`` [m] /
    ``normal_max_nn`` (3..64): the neighbourhood ``eval_collision.estimate_normals`` fits the target's normals in when none are
    given -- the radius must span a few point spacings (a point with fewer than 3 neighbours gets the normal (0, 0, 1)).

    ``association``: "nearest" (the grid search over any cloud) or "projective" (the lookup in the target's depth image, for
    a ``ProjectiveTarget``); the rest applies to the latter.  ``window`` (0..2): the candidates are the (2 window + 1)^2 pixels
    around the one a point falls on.  ``normal_angle`` [deg] in (0, 180], or None: a pair whose normals are further apart is
    refused (None: no test; the source then needs no normals).  ``normals``: where the organised cloud's normals come from --
    "image": ``depth_frame.normals``, differences ``normal_step`` (1..8) pixels along the image row and column that do not
    span a depth step of more than ``normal_jump`` [m]; "fit": ``estimate_normals`` over ``normal_radius`` on the finite rows,
    scattered back, slower and smoother (and one host read).  A one-pixel difference on a 640-wide frame spans about 3 mm at
    1 m, the size of depth noise: hence ``normal_step``.

    The defaults are choices -- a few millimetres and tenths of a degree of error in hand-measured extrinsics, a 2 cm capture
    range around them, a micrometre and ten microradians as "no longer moving"; a window of one pixel, a baseline of two, a
    depth step of the capture range -- and not measurements on real cameras."""
    WORD = "register"
    max_dist: float = 0.02
    iterations: int = 30
    stride: int = 1
    min_pairs: int = 100
    rot_eps: float = 1e-5
    trans_eps: float = 1e-6
    normal_radius: float = 0.02
    normal_max_nn: int = 30
    association: str = "nearest"
    window: int = 1
    normal_angle: Optional[float] = None
    normals: str = "image"
    normal_step: int = 2
    normal_jump: float = 0.02

    def __post_init__(self):
        for name in ("max_dist", "normal_radius", "normal_jump"):
            v = getattr(self, name)
            with np.errstate(over="ignore", under="ignore"):
                as32 = float(np.float32(v))
            if not (float(v) > 0.0 and np.isfinite(v) and 0.0 < as32 < np.inf):
                raise ValueError("register: %s must be positive and finite" % name)
        for name in ("rot_eps", "trans_eps"):
            v = getattr(self, name)
            if not (float(v) >= 0.0 and np.isfinite(v)):
                raise ValueError("register: %s must be non-negative and finite" % name)
        if int(self.iterations) != self.iterations or not 1 <= self.iterations <= MAX_ITERATIONS:
            raise ValueError("register: iterations must be in 1..%d" % MAX_ITERATIONS)
        if int(self.stride) != self.stride or self.stride < 1:
            raise ValueError("register: stride must be at least 1")
        if int(self.min_pairs) != self.min_pairs or self.min_pairs < 0:
            raise ValueError("register: min_pairs must be at least 0")
        if int(self.normal_max_nn) != self.normal_max_nn or not 3 <= self.normal_max_nn <= 64:
            raise ValueError("register: normal_max_nn must be in 3..64")
        if self.association not in ("nearest", "projective"):
            raise ValueError("register: association must be 'nearest' or 'projective'")
        if self.normals not in ("image", "fit"):
            raise ValueError("register: normals must be 'image' or 'fit'")
        if int(self.window) != self.window or not 0 <= self.window <= 2:
            raise ValueError("register: window must be 0, 1 or 2")
        if int(self.normal_step) != self.normal_step or not 1 <= self.normal_step <= 8:
            raise ValueError("register: normal_step must be in 1..8")
        if self.normal_angle is not None:
            if not 0.0 < float(self.normal_angle) <= 180.0:                   # (a NaN too)
                raise ValueError("register: normal_angle must be None or in (0, 180] degrees")
            if self.association == "nearest":
                raise ValueError("register: normal_angle needs association='projective' (the grid search has no normal test)")

    def min_cos(self):
        """The normal gate as the kernel takes it: cos(normal_angle), or -2 (below every cosine: the gate is off)."""
        return -2.0 if self.normal_angle is None else math.cos(math.radians(float(self.normal_angle)))


def _params(params):
    return IcpParams.coerce(params) or IcpParams()


def workspace_bytes(n_target, n_source):
    """Bytes of scratch of a registration: the target's grid and a slot of partial sums per 256 source rows; -1 beyond 2^21 rows."""
    return int(_L.regnet_icp_workspace_bytes(int(n_target), int(n_source)))


def initial_state(init=None, params=None):
    """The state block a registration starts from, as (1152,) uint8 on the host: the pose ``init`` (4x4, None: identity), zero
    iterations, RUNNING, and ``params``' limits (include/regnet_hip.h)."""
    params = _params(params)
    T = np.eye(4) if init is None else matrix4(init, "init must be a finite 4x4 source-to-target transform", finite=True)
    raw = np.zeros((STATE_BYTES,), dtype=np.uint8)
    raw[:96].view(np.float64)[:] = T[:3, :].reshape(12)
    raw[96:112].view(np.int32)[:] = (0, RUNNING, int(params.iterations), 0)
    raw[112:128].view(np.float64)[:] = (float(params.rot_eps), float(params.trans_eps))
    return raw


def decode_state(raw):
    """A state block's bytes -> dict: ``pose`` (4,4) float64, ``status``, ``iterations``, ``history`` (iterations, 2) float64 =
    (pairs, rms) per step, and the report row ``pairs`` (of the last step), ``rms_first``, ``rms_last`` (0 before any step)."""
    raw = np.ascontiguousarray(np.asarray(raw, dtype=np.uint8).reshape(STATE_BYTES))
    pose = np.eye(4)
    pose[:3, :] = raw[:96].view(np.float64).reshape(3, 4)
    iteration, status = (int(v) for v in raw[96:104].view(np.int32))
    history = raw[128:].view(np.float64).reshape(MAX_ITERATIONS, 2)[:min(iteration, MAX_ITERATIONS)].copy()
    ran = len(history) > 0
    return {"pose": pose, "status": status, "iterations": iteration, "history": history,
            "pairs": int(history[-1, 0]) if ran else 0, "rms_first": float(history[0, 1]) if ran else 0.0,
            "rms_last": float(history[-1, 1]) if ran else 0.0}


def report_row(decoded):
    """(status, iterations, pairs, rms first, rms last) of a decoded state."""
    return [float(decoded[k]) for k in ("status", "iterations", "pairs", "rms_first", "rms_last")]


class Target:
    """A target prepared for any number of registrations: ``xyz`` / ``normals`` (n,3) float32 on the device, the finite rows of
    the cloud it was made from; ``rows`` (n,) int64, their rows in that cloud; the workspace with the target's grid, good for
    sources of up to ``max_source`` rows at ``max_dist``."""

    def __init__(self, xyz, normals, rows, ws, max_source, max_dist):
        self.xyz, self.normals, self.rows, self.ws = xyz, normals, rows, ws
        self.n, self.max_source, self.max_dist = int(xyz.shape[0]), int(max_source), float(max_dist)


def prepare_target(target, params=None, target_normals=None, target_camera=(0.0, 0.0, 0.0), max_source=MAX_POINTS, stream=None):
    """``target`` (n,3) float32 on the device -> ``Target``: its finite rows compacted (one row count is read), their normals
    (``target_normals`` (n,3) float32, or estimated facing ``target_camera``) and the uniform grid, built once."""
    from . import eval_collision
    params = _params(params)
    require_cuda("target", target, torch.float32, 3)
    if target_normals is not None:
        require_cuda("target_normals", target_normals, torch.float32, 3)
        if target_normals.shape[0] != target.shape[0] or target_normals.device != target.device:
            raise ValueError("target_normals must have the target's rows and device")
    dev = target.device
    raw = None if stream is None else stream.cuda_stream
    with torch.cuda.device(dev), stream_scope(stream):
        finite = torch.isfinite(target).all(dim=1)
        rows = torch.nonzero(finite).reshape(-1)                    # the set-up's host read: the count of finite rows
        xyz = target.index_select(0, rows).contiguous()
        n = int(xyz.shape[0])
        if n < 1:
            raise ValueError("icp: the target has no finite row")
        if n > MAX_POINTS or max_source > MAX_POINTS:
            _lib.check(-3, "icp (at most 2^21 rows)")
        if target_normals is None:
            normals = eval_collision.estimate_normals(xyz, target_camera, params.normal_radius, params.normal_max_nn)
        else:
            normals = target_normals.index_select(0, rows).contiguous()
        ws = torch.empty((workspace_bytes(n, max_source),), dtype=torch.uint8, device=dev)
        _lib.call("regnet_icp_prepare_f32", ws, xyz.data_ptr(), n, float(params.max_dist), ws.data_ptr(), stream=raw)
        record_streams(stream, target, target_normals)
    return Target(xyz, normals, rows, ws, max_source, params.max_dist)


def projective_workspace_bytes(n_source):
    """Bytes of scratch of a projective registration: a slot of partial sums per 256 source rows; -1 beyond 2^21 rows."""
    return int(_L.regnet_icp_projective_workspace_bytes(int(n_source)))


class ProjectiveTarget:
    """A depth-frame target prepared for any number of projective registrations: ``xyz`` / ``normals`` (H W, 3) float32 on the
    device in the TARGET CAMERA's frame, row ``v W + u`` for pixel (u, v), NaN where a pixel was removed or has no normal;
    ``width``, ``height``; ``intrinsics`` (4,) float64 = (fx, fy, cx, cy) of that camera; the workspace, good for sources of up
    to ``max_source`` rows."""

    def __init__(self, xyz, normals, width, height, intrinsics, ws, max_source):
        self.xyz, self.normals, self.ws = xyz, normals, ws
        self.width, self.height, self.intrinsics, self.max_source = int(width), int(height), intrinsics, int(max_source)


def organised_normals(xyz, width, height, params=None, stream=None):
    """The normals of the organised cloud ``xyz`` (H W, 3) float32 on the device, in its camera's frame, by ``params.normals``:
    "image" -> ``depth_frame.normals`` (no host read); "fit" -> ``eval_collision.estimate_normals`` on the finite rows (their
    count is read), facing the camera, scattered back with NaN elsewhere."""
    from . import depth_frame, eval_collision
    params = _params(params)
    if params.normals == "image":
        return depth_frame.normals(xyz, width, height, params.normal_step, params.normal_jump, stream=stream)
    require_cuda("xyz", xyz, torch.float32, 3)
    if int(xyz.shape[0]) != int(width) * int(height):
        raise ValueError("normals: xyz must have width * height rows")
    with torch.cuda.device(xyz.device), stream_scope(stream):
        rows = torch.nonzero(torch.isfinite(xyz).all(dim=1)).reshape(-1)      # the host read of "fit": the count of finite rows
        out = torch.full_like(xyz, float("nan"))
        if int(rows.shape[0]) > 0:
            fitted = eval_collision.estimate_normals(xyz.index_select(0, rows).contiguous(), (0.0, 0.0, 0.0),
                                                     params.normal_radius, params.normal_max_nn)
            out.index_copy_(0, rows, fitted)
        record_streams(stream, xyz)
    return out


def prepare_projective_target(xyz, width, height, intrinsics, params=None, target_normals=None, max_source=MAX_POINTS,
                              stream=None):
    """``xyz`` (H W, 3) float32 on the device, the organised cloud of a ``width`` x ``height`` depth image in ITS camera's frame
    (``depth_frame.to_cloud``), and that camera's ``intrinsics`` (an ``Intrinsics`` or (fx, fy, cx, cy)) -> ``ProjectiveTarget``:
    the cloud as it is, its normals (``target_normals`` (H W, 3) float32, or ``organised_normals``) and the workspace.  Nothing is
    compacted and, with ``normals="image"``, nothing is read."""
    from . import depth_frame
    params = _params(params)
    require_cuda("target", xyz, torch.float32, 3)
    width, height = int(width), int(height)
    if width < 1 or height < 1 or int(xyz.shape[0]) != width * height:
        raise ValueError("icp: a projective target must have width * height rows")
    if width * height > MAX_POINTS or max_source > MAX_POINTS:
        _lib.check(-3, "icp (at most 2^21 rows)")
    k = np.array(depth_frame.Intrinsics.coerce(intrinsics).astuple(), dtype=np.float64)
    if not (np.isfinite(k).all() and k[0] > 0.0 and k[1] > 0.0):
        raise ValueError("icp: the intrinsics must be finite with positive fx and fy")
    xyz = xyz.contiguous()
    if target_normals is not None:
        require_cuda("target_normals", target_normals, torch.float32, 3)
        if target_normals.shape[0] != xyz.shape[0] or target_normals.device != xyz.device:
            raise ValueError("target_normals must have the target's rows and device")
        normals = target_normals.contiguous()
    else:
        normals = organised_normals(xyz, width, height, params, stream=stream)
    with torch.cuda.device(xyz.device), stream_scope(stream):
        ws = torch.empty((projective_workspace_bytes(max_source),), dtype=torch.uint8, device=xyz.device)
        record_streams(stream, xyz, target_normals)
    return ProjectiveTarget(xyz, normals, width, height, k, ws, max_source)


def step(source, target, state, params=None, idx_out=None, sums_out=None, stream=None, source_normals=None):
    """One iteration on ``state`` ((1152,) uint8 on the device), two launches, no host read.  ``source`` (n,3) float32 contiguous
    on the device; ``target`` a ``Target`` prepared at ``params.max_dist``, or a ``ProjectiveTarget`` (``params.association``
    must say "projective" then, and ``source_normals`` (n,3) float32 contiguous are needed with ``params.normal_angle``);
    ``idx_out`` (ceil(n / stride),) int32 and ``sums_out`` (29,) float64 on the device, or None."""
    params = _params(params)
    projective = isinstance(target, ProjectiveTarget)
    if not projective and not isinstance(target, Target):
        raise TypeError("step takes a prepared Target or ProjectiveTarget")
    if projective != (params.association == "projective"):
        raise ValueError("step: association = %r does not go with a %s" % (params.association, type(target).__name__))
    require_cuda("source", source, torch.float32, 3)
    if not source.is_contiguous() or source.device != target.xyz.device:
        raise ValueError("step: source must be contiguous and on the target's device (%s)" % target.xyz.device)
    if not isinstance(state, torch.Tensor) or not state.is_cuda or state.device != target.xyz.device:
        raise RuntimeError("step: state must be a CUDA tensor on the target's device")
    for name, t in (("idx_out", idx_out), ("sums_out", sums_out)):
        if t is not None and (not t.is_cuda or t.device != target.xyz.device):
            raise RuntimeError("step: %s must be a CUDA tensor on the target's device" % name)
    if not projective and float(params.max_dist) != target.max_dist:
        raise ValueError("step: the target was prepared at max_dist = %g" % target.max_dist)
    n = int(source.shape[0])
    if n > target.max_source:
        raise ValueError("step: the target's workspace is sized for %d source rows" % target.max_source)
    rows = (n + int(params.stride) - 1) // int(params.stride)
    if idx_out is not None and (idx_out.dtype != torch.int32 or idx_out.numel() < rows or not idx_out.is_contiguous()):
        raise ValueError("idx_out must be contiguous int32 with a row per visited source row")
    if sums_out is not None and (sums_out.dtype != torch.float64 or sums_out.numel() < 29 or not sums_out.is_contiguous()):
        raise ValueError("sums_out must be contiguous float64 (29)")
    if state.dtype != torch.uint8 or state.numel() != STATE_BYTES or not state.is_contiguous():
        raise ValueError("state must be contiguous uint8 (%d)" % STATE_BYTES)
    raw = None if stream is None else stream.cuda_stream
    if projective:
        gate = params.normal_angle is not None
        if gate:
            if source_normals is None:
                raise ValueError("step: normal_angle needs source_normals")
            require_cuda("source_normals", source_normals, torch.float32, 3)
            if (source_normals.shape[0] != n or not source_normals.is_contiguous() or source_normals.device != source.device):
                raise ValueError("step: source_normals must be contiguous with the source's rows and device")
        _lib.call("regnet_icp_step_projective_f32", target.ws, source.data_ptr(), n, int(params.stride),
                  source_normals.data_ptr() if gate else None, target.xyz.data_ptr(), target.normals.data_ptr(), target.width,
                  target.height, target.intrinsics.ctypes.data, int(params.window), state.data_ptr(), float(params.max_dist),
                  float(params.min_cos()), None if idx_out is None else idx_out.data_ptr(),
                  None if sums_out is None else sums_out.data_ptr(), int(params.min_pairs), target.ws.data_ptr(), stream=raw)
        return
    _lib.call("regnet_icp_step_f32", target.ws, source.data_ptr(), n, int(params.stride), target.normals.data_ptr(), target.n,
              state.data_ptr(), float(params.max_dist), None if idx_out is None else idx_out.data_ptr(),
              None if sums_out is None else sums_out.data_ptr(), int(params.min_pairs), target.ws.data_ptr(), stream=raw)


def continue_state(state, budget, mark=None, stream=None):
    """The hand-over of ``state`` ((1152,) uint8 on the device) between two levels of a coarse-to-fine registration
    (regnet_icp_state_continue): ``mark`` ((2,) int32 on the device, or None) takes ``(iteration, status)`` as found; a block that
    ended CONVERGED or MAX_ITER is RUNNING again for at most ``budget`` (1..64) more steps, 64 in all, with its pose and history;
    any other status stays, so a registration that ended TOO_FEW or DEGENERATE on a coarse level stays ended.  One launch of one
    thread, no host read."""
    if not isinstance(state, torch.Tensor) or not state.is_cuda:
        raise RuntimeError("continue_state: state must be a CUDA tensor")
    if state.dtype != torch.uint8 or state.numel() != STATE_BYTES or not state.is_contiguous():
        raise ValueError("state must be contiguous uint8 (%d)" % STATE_BYTES)
    if int(budget) != budget or not 1 <= budget <= MAX_ITERATIONS:
        raise ValueError("continue_state: budget must be in 1..%d" % MAX_ITERATIONS)
    if mark is not None:
        if not isinstance(mark, torch.Tensor) or not mark.is_cuda or mark.device != state.device:
            raise RuntimeError("continue_state: mark must be a CUDA tensor on the state's device")
        if mark.dtype != torch.int32 or mark.numel() != 2 or not mark.is_contiguous():
            raise ValueError("mark must be contiguous int32 (2)")
    _lib.call("regnet_icp_state_continue", state, state.data_ptr(), int(budget), None if mark is None else mark.data_ptr(),
              stream=None if stream is None else stream.cuda_stream)


class Registration:
    """``icp``'s result: ``state``, the (1152,) uint8 device block, and what ``result()`` reads from it."""

    def __init__(self, state, init, params):
        self.state, self.init, self.params = state, init, params
        self._decoded = None

    def result(self):
        """The one blocking read, 1152 bytes -> ``decode_state``'s dict (kept: later calls read nothing)."""
        if self._decoded is None:
            self._decoded = decode_state(self.state.cpu().numpy())
        return self._decoded

    def pose(self):
        """The refined source-to-target transform, (4,4) float64."""
        return self.result()["pose"].copy()

    status = property(lambda self: self.result()["status"])
    iterations = property(lambda self: self.result()["iterations"])
    pairs = property(lambda self: self.result()["pairs"])
    rms_first = property(lambda self: self.result()["rms_first"])
    rms_last = property(lambda self: self.result()["rms_last"])


def icp(source, target, init=None, params=None, target_normals=None, target_camera=(0.0, 0.0, 0.0), stream=None, state=None,
        source_normals=None, source_shape=None):
    """Register ``source`` (n,3) float32 on the device onto ``target`` ((m,3) float32 on the device, a ``Target`` or a
    ``ProjectiveTarget``) starting from the pose ``init`` (4x4 source-to-target, None: identity) -> ``Registration``.
    ``params``: an ``IcpParams``, a dict of its fields or None; ``target_normals`` (m,3) float32 or None (estimated, facing
    ``target_camera``); ``stream``: a ``torch.cuda.Stream`` (default: the current one); ``state``: a (1152,) uint8 device block
    ALREADY holding ``initial_state`` to run on instead of a new one.  ``iterations`` steps are enqueued; nothing is read after
    the target is prepared.  With ``association="projective"`` the target must be a ``ProjectiveTarget`` and the pose is source
    to TARGET CAMERA; with ``normal_angle`` the source's normals are ``source_normals`` (n,3) float32 in the source's frame, or
    are made by ``organised_normals`` from the organised source of ``source_shape`` = (width, height)."""
    params = _params(params)
    require_cuda("source", source, torch.float32, 3)
    if params.association == "projective":
        if not isinstance(target, ProjectiveTarget):
            raise ValueError("register: association='projective' takes a ProjectiveTarget (prepare_projective_target)")
        if int(source.shape[0]) > target.max_source:
            raise ValueError("icp: the target's workspace is sized for %d source rows" % target.max_source)
    elif isinstance(target, ProjectiveTarget):
        raise ValueError("register: a ProjectiveTarget needs association='projective'")
    elif not isinstance(target, Target):
        target = prepare_target(target, params, target_normals, target_camera, max_source=int(source.shape[0]), stream=stream)
    if source.device != target.xyz.device:
        raise RuntimeError("icp: source is on %s, the target on %s" % (source.device, target.xyz.device))
    init = np.eye(4) if init is None else matrix4(init, "init must be a finite 4x4 source-to-target transform", finite=True)
    source = source.contiguous()
    if params.normal_angle is not None:
        if source_normals is None:
            if source_shape is None:
                raise ValueError("register: normal_angle needs source_normals, or source_shape = (width, height) to make them")
            source_normals = organised_normals(source, int(source_shape[0]), int(source_shape[1]), params, stream=stream)
        else:
            require_cuda("source_normals", source_normals, torch.float32, 3)
            source_normals = source_normals.contiguous()
    else:
        source_normals = None
    with torch.cuda.device(source.device), stream_scope(stream):
        if state is None:
            state = to_device(initial_state(init, params), source.device)
        for _ in range(int(params.iterations)):
            step(source, target, state, params, stream=stream, source_normals=source_normals)
        record_streams(stream, source, state, source_normals)
    return Registration(state, init, params)
