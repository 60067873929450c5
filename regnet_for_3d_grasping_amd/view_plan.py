"""Next-best view (csrc/view_gain.hip): rank candidate camera poses by the unobserved volume they would reveal.

The TSDF volume (``tsdf.Volume``) knows three states per voxel -- seen solid, seen free, never observed -- and the approach
analysis reports the third: a grasp whose hand or retreat passes through unobserved space is rejected by ``unseen="blocked"``
and stays rejected.  ``view_gain`` answers the question that follows for a camera that can move: from which pose would that
space become observed?  A coarse virtual camera at every candidate pose marches its rays through the volume and marks the
unobserved voxels they reach before a solid voxel, or ``max_unknown`` samples of unobserved matter, stops them; ``ViewGain.pick``
then chooses K poses JOINTLY and greedily, so that the second pick adds what the first does not already cover.  ``interest_hands``
restricts the count to the unobserved voxels inside the swept hands of analysed grasps, ``interest_box`` to a box.

It is a count of voxels, not a measurement: unobserved matter is transparent for ``max_unknown`` samples and opaque after, the
samples are a fixed step apart and read the nearest voxel, nothing is weighted by distance or incidence, and the candidates of
``orbit_poses`` know nothing of what a robot can reach (DESIGN.md par. 10).  The arithmetic is pinned (include/regnet_hip.h
"next-best view"), so ``tests/view_gain_reference.py`` restates it in numpy and the two agree bit for bit.  Nothing here reads
from the device or waits for it except ``ViewGain.to_host``.  GPU only: there is no CPU path.
"""
import math
from dataclasses import dataclass
from typing import Optional, Tuple

import numpy as np
import torch

from . import _lib, approach, approach_volume, depth_frame, tsdf
from ._frame_util import ParamsBase, matrix4, record_streams, require_cuda, stream_scope, to_device

MAX_POSES = 32                      # regnet_tsdf_view_mark_f32's documented limits: a pose is a bit of a 32-bit word
MAX_RAY_STEPS = 4096
STATE_WORDS = 64                    # REGNET_VIEW_PICK_STATE_WORDS
EXITED, BLOCKED, SATURATED = 0, 1, 2      # ``ViewGain.status``; columns 0..2 of ``rays``, column 3: rays with a bit request
INTERESTS = ("all", "grasps")


@dataclass(frozen=True)
class ViewParams(ParamsBase):
    """What ``GraspDetector(view=...)`` takes (a dict with these keys works too).  ``width`` x ``height``: the virtual camera's
    image, its intrinsics scaled from the frame's; ``near`` / ``far`` [m]: the depth range of a ray; ``step`` [m]: the distance
    between two samples (None: the volume's voxel); ``max_unknown``: a ray ends after so many samples in unobserved voxels (None:
    the samples in 5 cm); ``margin`` [m]: a voxel is solid when its distance is below it (``approach``'s); ``top_k``: the poses
    picked jointly; ``min_gain``: a pick that adds fewer voxels ends the order; ``interest``: ``"all"`` unobserved voxels count,
    or ``"grasps"``: only those inside the swept hands of the analysed grasps.  The candidates: ``azimuths`` x ``elevations`` poses
    (at most 32) on a sphere of ``radius`` [m] about the target, the elevations spread over ``elevation_deg`` above the plane
    whose normal is ``up`` (common frame; the first camera looks along +z with y down, so "up" is -y).

    Every default is a choice: a coarse image whose pixels are about a voxel apart at arm's length, unobserved matter opaque after
    5 cm, an orbit at half a metre.  Nobody has measured them on a robot."""
    WORD = "view"
    width: int = 80
    height: int = 60
    near: float = 0.1
    far: float = 1.0
    step: Optional[float] = None
    max_unknown: Optional[int] = None
    margin: float = 0.0
    top_k: int = 4
    min_gain: int = 0
    interest: str = "all"
    azimuths: int = 8
    elevations: int = 2
    radius: float = 0.5
    elevation_deg: Tuple[float, float] = (30.0, 60.0)
    up: Tuple[float, float, float] = (0.0, -1.0, 0.0)

    def __post_init__(self):
        for name in ("width", "height", "top_k", "azimuths", "elevations"):
            if int(getattr(self, name)) != getattr(self, name) or getattr(self, name) < 1:
                raise ValueError("view: %s must be a positive integer" % name)
        if self.azimuths * self.elevations > MAX_POSES:
            raise ValueError("view: at most %d candidate poses (azimuths x elevations)" % MAX_POSES)
        if self.top_k > self.azimuths * self.elevations:
            raise ValueError("view: top_k cannot exceed the number of candidates")
        tsdf.check_ray_range(self.near, self.far, self.step, "view")
        if self.max_unknown is not None and (int(self.max_unknown) != self.max_unknown or self.max_unknown < 1):
            raise ValueError("view: max_unknown must be None or a positive integer")
        if int(self.min_gain) != self.min_gain or self.min_gain < 0:
            raise ValueError("view: min_gain must be a non-negative integer")
        if not np.isfinite(self.margin):
            raise ValueError("view: margin must be finite")
        if self.interest not in INTERESTS:
            raise ValueError("view: interest must be one of %s, not %r" % (", ".join(INTERESTS), self.interest))
        if not (float(self.radius) > 0.0 and np.isfinite(self.radius)):
            raise ValueError("view: radius must be positive and finite")
        lo, hi = (float(v) for v in self.elevation_deg)
        if not -90.0 < lo <= hi < 90.0:
            raise ValueError("view: elevation_deg must be (lo, hi) with -90 < lo <= hi < 90")
        object.__setattr__(self, "elevation_deg", (lo, hi))
        up = tuple(float(v) for v in self.up)
        if len(up) != 3 or not np.isfinite(up).all() or not np.linalg.norm(up) > 0.0:
            raise ValueError("view: up must be a finite, non-zero 3-vector")
        object.__setattr__(self, "up", up)

    def angles(self):
        """-> (azimuths, elevations) in degrees: the azimuths evenly round the circle, the elevations evenly over
        ``elevation_deg`` (its middle when there is one)."""
        lo, hi = self.elevation_deg
        az = [360.0 * j / self.azimuths for j in range(self.azimuths)]
        el = [0.5 * (lo + hi)] if self.elevations == 1 else [lo + (hi - lo) * j / (self.elevations - 1) for j in range(self.elevations)]
        return az, el

    def scaled_intrinsics(self, intrinsics, width, height):
        """The frame's ``intrinsics`` for its ``width`` x ``height`` image -> those of this ``width`` x ``height`` image of the
        same field of view: the focal lengths scale with the image, the centre keeps its place between the pixel centres."""
        k = depth_frame.Intrinsics.coerce(intrinsics)
        sx, sy = self.width / float(width), self.height / float(height)
        return depth_frame.Intrinsics(k.fx * sx, k.fy * sy, (k.cx + 0.5) * sx - 0.5, (k.cy + 0.5) * sy - 0.5)


def orbit_poses(target, radius, azimuths, elevations, up=(0.0, -1.0, 0.0)):
    """Candidate poses on a sphere cap about ``target`` (3), looking at it -> (P,4,4) float64 camera-to-common, P =
    len(elevations) len(azimuths), elevation-major.  ``azimuths`` / ``elevations``: degrees, round ``up`` and above the plane it is
    normal to, |elevation| < 90.  The project's camera convention (``depth_frame.to_cloud``): z forward, x right, y down -- ``up``
    is the direction the image's top points to.  Host, float64."""
    target = np.asarray(target, dtype=np.float64).reshape(3)
    n = np.asarray(up, dtype=np.float64).reshape(3)
    if not (np.isfinite(target).all() and np.isfinite(n).all() and np.linalg.norm(n) > 0.0 and float(radius) > 0.0
            and np.isfinite(radius)):
        raise ValueError("orbit_poses: target and up must be finite, up non-zero, radius positive")
    n = n / np.linalg.norm(n)
    e1 = np.cross(n, [1.0, 0.0, 0.0] if abs(n[0]) < 0.9 else [0.0, 0.0, 1.0])
    e1 /= np.linalg.norm(e1)
    e2 = np.cross(n, e1)
    poses = []
    for el in np.asarray(elevations, dtype=np.float64).reshape(-1):
        if not abs(el) < 90.0:
            raise ValueError("orbit_poses: an elevation must lie strictly between -90 and 90 degrees")
        for az in np.asarray(azimuths, dtype=np.float64).reshape(-1):
            a, e = math.radians(az), math.radians(el)
            at = target + float(radius) * (math.cos(e) * (math.cos(a) * e1 + math.sin(a) * e2) + math.sin(e) * n)
            z = (target - at) / np.linalg.norm(target - at)
            x = np.cross(-n, z)
            x /= np.linalg.norm(x)
            y = np.cross(z, x)
            T = np.eye(4)
            T[:3, 0], T[:3, 1], T[:3, 2], T[:3, 3] = x, y, z, at
            poses.append(T)
    if not poses:
        raise ValueError("orbit_poses: no azimuth or no elevation")
    return np.stack(poses)


class ViewGain:
    """``view_gain``'s result, on the device: ``plane`` (N) int32 -- bit p of word l is set iff a ray of pose p reached the
    unobserved (and wanted) voxel l; it is the VOLUME's scratch plane, valid until the next ``view_gain`` on that volume --
    ``rays`` (P,4) int32 = per pose the rays that EXITED, were BLOCKED, SATURATED, and that requested at least one bit;
    ``status`` (P, H W) uint8 or None; ``poses``: (P,4,4) float64 on the host, or the device rows, as given."""

    def __init__(self, plane, rays, status, poses, width, height, volume):
        self.plane, self.rays, self.status, self.poses = plane, rays, status, poses
        self.width, self.height, self.volume = int(width), int(height), volume
        self.P = int(rays.shape[0])
        self._gain = None

    def pick(self, k=1, min_gain=0, stream=None):
        """The greedy joint selection of ``k`` of the poses -> (``order`` (k) int32: the pose picked in every round, -1 from the
        round on in which the best pose adds fewer than ``max(min_gain, 1)`` voxels; ``order_gain`` (k) int32: what each pick
        adds to the picks before it).  A fill and 2 k launches, no host read."""
        k, min_gain = int(k), int(min_gain)
        if not 1 <= k <= self.P or min_gain < 0:
            raise ValueError("pick: k must be in 1..%d and min_gain non-negative" % self.P)
        dev = self.plane.device
        with torch.cuda.device(dev), stream_scope(stream):
            state = torch.empty((STATE_WORDS,), dtype=torch.int32, device=dev)
            gain = torch.empty((self.P,), dtype=torch.int32, device=dev)
            order = torch.empty((k,), dtype=torch.int32, device=dev)
            order_gain = torch.empty((k,), dtype=torch.int32, device=dev)
            _lib.call("regnet_tsdf_view_pick", self.plane, self.plane.data_ptr(), int(self.plane.numel()), self.P, k, min_gain,
                      state.data_ptr(), gain.data_ptr(), order.data_ptr(), order_gain.data_ptr(),
                      stream=None if stream is None else stream.cuda_stream)
            record_streams(stream, self.plane, state, gain, order, order_gain)
        self._gain = gain
        return order, order_gain

    def gain(self, stream=None):
        """(P) int32: per pose the voxels it marked, alone.  The first round of a pick counts it; kept after the first call."""
        if self._gain is None:
            self.pick(1, stream=stream)
        return self._gain

    def to_host(self, k=1, min_gain=0):
        """The one blocking read -> dict of numpy arrays: ``gain`` (P), ``rays`` (P,4), ``order`` (k), ``order_gain`` (k) int32."""
        order, order_gain = self.pick(k, min_gain)
        flat = torch.cat([self._gain, self.rays.reshape(-1), order, order_gain]).cpu().numpy()
        P = self.P
        return {"gain": flat[:P].copy(), "rays": flat[P:5 * P].reshape(P, 4).copy(), "order": flat[5 * P:5 * P + len(order)].copy(),
                "order_gain": flat[5 * P + len(order):].copy()}


def pose_rows(poses):
    """``poses``: (P,4,4) finite camera-to-common transforms (array or tensor), or one 4x4 -> ((P,4,4) float64 host array, (P,12)
    float32 host array: rows 0..2 of each, rounded once)."""
    T = np.asarray(poses.detach().cpu().numpy() if hasattr(poses, "detach") else poses, dtype=np.float64)
    if T.shape == (4, 4):
        T = T[None]
    if T.ndim != 3 or T.shape[1:] != (4, 4) or not np.isfinite(T).all():
        raise ValueError("view_gain: poses must be finite (P,4,4) camera-to-common transforms")
    if not 1 <= T.shape[0] <= MAX_POSES:
        raise ValueError("view_gain: %d poses; a call takes 1..%d (a pose is a bit of the plane's words)" % (T.shape[0], MAX_POSES))
    with np.errstate(over="ignore"):
        return T, np.ascontiguousarray(T[:, :3, :].reshape(-1, 12).astype(np.float32))


def default_max_unknown(step, n_steps):
    """The samples in 5 cm of a ray, at least 1 and at most ``n_steps``."""
    return max(1, min(int(n_steps), int(math.ceil(0.05 / float(step)))))


def view_gain(volume, poses, intrinsics, width, height, near=None, far=None, step=None, max_unknown=None, margin=0.0,
              interest=None, status=True, clip=True, stream=None, out=None):
    """``Volume.view_gain``: mark, per candidate pose, the unobserved voxels of ``volume`` its rays reach -> ``ViewGain``.
    ``poses`` (P,4,4) camera-to-common on the host, or their rows 0..2 as (P,12) float32 already on the device, P <= 32, more
    raises; ``intrinsics`` (an ``Intrinsics`` or (fx, fy, cx, cy)) for the
    ``width`` x ``height`` image; ``near`` / ``far`` / ``step`` / ``max_unknown`` / ``margin``: ``ViewParams``' (None: its
    defaults); ``interest``: (N) uint8 on the device (``interest_hands``, ``interest_box``) or None: every unobserved voxel
    counts; ``status`` False: no per-ray status; ``clip`` False visits every sample: the same bytes, more time (a measurement);
    ``out``: ``(rays, status)`` contiguous device tensors of the result's shapes (status None without it).  The plane, 4 bytes per
    voxel, is allocated on the first call and kept on the volume; the poses go up in one copy.  Two fills and one launch, no
    host read; the volume is only read."""
    p = volume.params
    width, height = int(width), int(height)
    k = depth_frame.Intrinsics.coerce(intrinsics)
    if k is None or not (np.isfinite(k.astuple()).all() and k.fx != 0.0 and k.fy != 0.0):
        raise ValueError("view_gain: the intrinsics must be finite with non-zero fx and fy")
    if width < 1 or height < 1:
        raise ValueError("view_gain: width and height must be at least 1")
    defaults = ViewParams()
    near = defaults.near if near is None else near
    far = defaults.far if far is None else far
    step = float(p.voxel) if step is None else step
    tsdf.check_ray_range(near, far, step, "view_gain")
    n_steps = tsdf.ray_steps(near, far, step)
    if n_steps > MAX_RAY_STEPS:
        raise ValueError("view_gain: %d samples per ray, more than %d; raise step or bring near and far together"
                         % (n_steps, MAX_RAY_STEPS))
    max_unknown = default_max_unknown(step, n_steps) if max_unknown is None else int(max_unknown)
    if not 1 <= max_unknown <= n_steps:
        raise ValueError("view_gain: max_unknown must be in 1..%d, the samples of a ray" % n_steps)
    dev = volume.device
    if isinstance(poses, torch.Tensor) and poses.is_cuda:      # rows already on the device: nothing is uploaded (a captured call)
        require_cuda("poses", poses, torch.float32, 12, error=TypeError)
        if poses.device != dev or not poses.is_contiguous() or not 1 <= int(poses.shape[0]) <= MAX_POSES:
            raise ValueError("view_gain: device poses must be contiguous (P,12) float32 rows on the volume's device, P in 1..%d"
                             % MAX_POSES)
        T = rows = poses
    else:
        T, rows = pose_rows(poses)
    P = int(T.shape[0])
    with np.errstate(over="ignore"):
        k4 = np.ascontiguousarray(np.array([1.0 / k.fx, 1.0 / k.fy, k.cx, k.cy], dtype=np.float64).astype(np.float32))
    nx, ny, nz = p.dims
    n = nx * ny * nz
    if interest is not None:
        require_cuda("interest", interest, torch.uint8, error=TypeError)
        if interest.device != dev or int(interest.numel()) != n or not interest.is_contiguous():
            raise ValueError("view_gain: interest must be a contiguous (N) uint8 tensor on the volume's device")
    with torch.cuda.device(dev), stream_scope(stream):
        if getattr(volume, "view_plane", None) is None:
            volume.view_plane = torch.empty((n,), dtype=torch.int32, device=dev)
        plane = volume.view_plane
        if out is None:
            out = (torch.empty((P, 4), dtype=torch.int32, device=dev),
                   torch.empty((P, width * height), dtype=torch.uint8, device=dev) if status else None)
        rays, state = out
        shapes = ((rays, (P, 4), torch.int32),) + (((state, (P, width * height), torch.uint8),) if status else ())
        if (state is None) != (not status) or any(not (t.is_cuda and t.device == dev and tuple(t.shape) == shape
                                                       and t.dtype == dtype and t.is_contiguous()) for t, shape, dtype in shapes):
            raise ValueError("view_gain: out must be (rays (P,4) int32, status (P, H W) uint8 or None) contiguous on the device")
        device_rows = to_device(rows, dev)
        _lib.call("regnet_tsdf_view_mark_f32", volume.data, volume.data.data_ptr(), nx, ny, nz, volume.origin.ctypes.data,
                  float(p.voxel), float(p.trunc), int(p.min_weight), float(margin), k4.ctypes.data, device_rows.data_ptr(), P,
                  float(near), float(step), n_steps, width, height, 1 if clip else 0, max_unknown,
                  None if interest is None else interest.data_ptr(), plane.data_ptr(), None if state is None else state.data_ptr(),
                  rays.data_ptr(), stream=None if stream is None else stream.cuda_stream)
        record_streams(stream, volume.data, plane, device_rows, interest, rays, state)
    return ViewGain(plane, rays, state, T, width, height, volume)


def interest_hands(volume, grasp, depth, width, params=None, to_volume=None, max_depth=None, out=None, rows=None):
    """The unobserved voxels inside the swept hands of ``grasp`` -> (``interest`` (N) uint8 on the device: 1 there, else 0;
    ``counts`` (B) int32: the unobserved samples per grasp).  The arguments are ``approach.analyse_volume``'s and so are the
    lattice, the sets and the lookup (``params``: ``standoff``, ``step`` and ``margin`` are read); ``out``: an (N) uint8 tensor
    to clear and write instead of a new one; ``rows``: the ``L`` (B,12) an analysis of the same grasps formed
    (``VolumeApproach.L``), which is then not formed again.  One fill and one launch, no host read."""
    params = approach.ApproachParams.coerce(params) or approach.ApproachParams()
    p = volume.params
    dev, B, depth, x_extent = approach_volume.hand_call("interest_hands", volume, grasp, depth, max_depth)
    L = approach_volume.local_to_volume(grasp, to_volume)[3] if rows is None else rows
    box, keep, step, _ = approach_volume.hand_lattice("interest_hands", volume, depth, width, B, params.step, params.standoff, x_extent)
    nx, ny, nz = p.dims
    n = nx * ny * nz
    if out is None:
        out = torch.zeros((n,), dtype=torch.uint8, device=dev)
    else:
        if not (out.is_cuda and out.device == dev and tuple(out.shape) == (n,) and out.dtype == torch.uint8 and out.is_contiguous()):
            raise ValueError("interest_hands: out must be a contiguous (N) uint8 tensor on the volume's device")
        out.zero_()
    counts = torch.empty((B,), dtype=torch.int32, device=dev)
    _lib.call("regnet_tsdf_view_interest_hands", volume.data, volume.data.data_ptr(), nx, ny, nz, volume.origin.ctypes.data,
              float(p.voxel), float(p.trunc), int(p.min_weight), float(params.margin), L.data_ptr(), B, *box,
              float(params.standoff), step, x_extent, out.data_ptr(), counts.data_ptr())
    return out, counts


def interest_box(volume, lo, hi):
    """The voxels whose centre lies in the box [``lo``, ``hi``] of the volume's frame -> ``interest`` (N) uint8 on the device.
    torch ops on three index vectors; nothing is read back."""
    p = volume.params
    lo, hi = np.asarray(lo, dtype=np.float64).reshape(3), np.asarray(hi, dtype=np.float64).reshape(3)
    if not (np.isfinite(lo).all() and np.isfinite(hi).all()):
        raise ValueError("interest_box: lo and hi must be finite 3-vectors")
    inside = []
    for axis, count in enumerate(p.dims):
        centre = float(volume.origin[axis]) + (torch.arange(count, dtype=torch.float64, device=volume.device) + 0.5) * float(p.voxel)
        inside.append((centre >= float(lo[axis])) & (centre <= float(hi[axis])))
    box = inside[2][:, None, None] & inside[1][None, :, None] & inside[0][None, None, :]
    return box.reshape(-1).to(torch.uint8).contiguous()


VIEW_KEYS = ("view_pose", "view_gain", "view_rays", "view_order", "view_order_gain")


def plan(volume, params, target, intrinsics, interest=None):
    """The detector's stage: ``orbit_poses`` about ``target`` (volume frame), ``view_gain`` and the joint pick -> the record's
    ``VIEW_KEYS`` as numpy arrays (one blocking read).  ``intrinsics``: those of the virtual image (``scaled_intrinsics``)."""
    azimuths, elevations = params.angles()
    poses = orbit_poses(target, params.radius, azimuths, elevations, params.up)
    result = view_gain(volume, poses, intrinsics, params.width, params.height, params.near, params.far, params.step,
                       params.max_unknown, params.margin, interest=interest, status=False)
    host = result.to_host(params.top_k, params.min_gain)
    return dict(zip(VIEW_KEYS, (poses, host["gain"], host["rays"], host["order"], host["order_gain"])))
