"""Several depth views, one surface (csrc/tsdf.hip): a truncated signed distance volume on the device, the KinectFusion
representation.

``Volume.integrate`` takes the organised cloud ``depth_frame.to_cloud`` leaves on the device -- so the flying-pixel filter, the
range gate and the registered colours are reused -- and the view's pose, and updates every voxel the view sees: the running mean
of the truncated distance to the surface along the viewing ray, the running mean colour, the observation count.  Noise along the
ray averages out, a view that looks THROUGH a voxel says that it is empty, and ``Volume.extract`` returns the zero crossings of
the distance with the normals of its gradient: one row per crossed voxel edge, in ascending order of the key ``3 * linear(voxel)
+ axis``, with no sort.  One thread owns one voxel, every operation is an individually rounded float32 one in a written order
(include/regnet_hip.h, DESIGN.md par. 5), so ``tests/tsdf_reference.py`` restates it in numpy and the two agree bit for bit; the
order of the views is the order of the calls and is part of the result.  The volume persists across calls: one camera, many
frames, and with a finite ``max_weight`` a moving average.

``fuse_volume`` is the counterpart of ``fusion.fuse_frames`` for a ``fusion.MultiView``, and ``GraspDetector(volume=...)`` uses
it.  No host read except ``Surface.check()``; GPU only: there is no CPU path.
"""
from dataclasses import dataclass
from typing import Tuple

import numpy as np

from . import _lib, depth_frame
from ._frame_util import MAX_FRAME_POINTS, ParamsBase, matrix4, record_streams, require_cuda, stream_scope

_L = _lib.lib

MAX_VOLUME_VOXELS = 1 << 28         # regnet_tsdf_*'s documented limits
MAX_POINTS = MAX_FRAME_POINTS
BLOCK = 256                         # voxels per workgroup of the two extraction passes
UPDATED, NOT_IN_VIEW, NO_DEPTH, BEHIND = 0, 1, 2, 3      # the entries of integrate's counts


@dataclass(frozen=True)
class TsdfParams(ParamsBase):
    """What ``GraspDetector(volume=...)`` takes (a dict with these keys works too).  ``voxel``: the voxel edge [m]; ``trunc``: the
    truncation distance [m], at least two voxels, so that a surface always has an observed voxel on either side; ``origin``: the
    corner of voxel (0, 0, 0) in the common frame; ``dims``: voxels per axis, at most 2^28 in all; ``max_weight``: the observation
    count saturates there, and the running mean becomes a moving average; ``min_weight``: a voxel bounds a surface only when it
    was observed so often (2 and more: what one view alone saw is dropped); ``max_points``: the rows of the surface, at most 2^21
    -- one that has more sets the overflow flag.

    Every default is a choice: a 64 cm cube in front of the first camera, at about the point spacing of a 640 x 480 frame at 1 m.
    None is measured on real cameras."""
    WORD = "volume"
    voxel: float = 0.002
    trunc: float = 0.01
    origin: Tuple[float, float, float] = (-0.32, -0.32, 0.3)
    dims: Tuple[int, int, int] = (320, 320, 320)
    max_weight: int = 255
    min_weight: int = 1
    max_points: int = 1 << 20

    def __post_init__(self):
        for name in ("voxel", "trunc"):
            with np.errstate(over="ignore"):
                value = np.float32(getattr(self, name))
            if not (value > 0.0 and np.isfinite(value)):
                raise ValueError("volume: %s must be positive and finite in float32" % name)
        if not float(self.trunc) >= 2.0 * float(self.voxel):
            raise ValueError("volume: trunc must be at least two voxels")
        origin = tuple(float(v) for v in self.origin)
        if len(origin) != 3 or not all(np.isfinite(v) for v in origin):
            raise ValueError("volume: origin must be three finite values")
        object.__setattr__(self, "origin", origin)
        dims = tuple(self.dims)
        if len(dims) != 3 or any(int(d) != d or d < 1 for d in dims):
            raise ValueError("volume: dims must be three positive integers")
        dims = tuple(int(d) for d in dims)
        if dims[0] * dims[1] * dims[2] > MAX_VOLUME_VOXELS:
            raise ValueError("volume: at most 2^28 voxels")
        object.__setattr__(self, "dims", dims)
        for name in ("max_weight", "min_weight"):
            if int(getattr(self, name)) != getattr(self, name) or not 1 <= getattr(self, name) < 1 << 31:
                raise ValueError("volume: %s must be at least 1" % name)
        if int(self.max_points) != self.max_points or not 1 <= self.max_points <= MAX_POINTS:
            raise ValueError("volume: max_points must be in 1..2^21")


class Surface:
    """``Volume.extract``'s result, all on the device and ``max_points`` rows long: ``xyz`` / ``rgb`` / ``normal`` (max_points,3)
    float32, NaN / 0 / NaN beyond the ``K`` rows; ``weight`` (max_points) int32, the smaller observation count of the two voxels
    of the row's edge, -1 beyond ``K``; ``num`` (4) int32 = (K, kept candidates in all, voxels observed ``min_weight`` times,
    overflow)."""

    def __init__(self, xyz, rgb, normal, weight, num, params):
        self.xyz, self.rgb, self.normal, self.weight, self.num, self.params = xyz, rgb, normal, weight, num, params
        self.counts = None                      # set by fuse_volume: (views,4) int32 on the device, integrate's histograms
        self.poses = self.register = None       # set by fuse_volume(register=...): the refined poses and refine_poses' report
        self.volume = None                      # set by fuse_volume: the Volume the surface was taken from

    def check(self):
        """The one blocking read, 16 bytes -> (K, kept candidates, observed voxels).  Raises ``ValueError`` when the surface
        overflowed: the rows are then only those of the ``max_points`` smallest keys."""
        k, total, observed, overflow = (int(v) for v in self.num.cpu())
        if overflow:
            raise ValueError("tsdf: the surface has %d rows, more than max_points = %d; raise max_points (at most 2^21) or the "
                             "voxel size" % (total, self.params.max_points))
        return k, total, observed

    def cloud(self):
        """The ``(xyz, rgb)`` pair ``ingest.ingest_frame``, ``table_plane.calibrate`` and ``outliers.filter_cloud`` take as they
        are: the rows beyond ``K`` are NaN rows, which all three treat as absent."""
        return self.xyz, self.rgb


def camera_from_common(pose):
    """A view's pose -- the row-major 4x4 camera-to-common transform, None: identity -> the first three rows of its inverse as 12
    float32: inverted in float64, each entry rounded once."""
    T = np.eye(4) if pose is None else matrix4(pose, "a pose must be a finite 4x4 camera-to-common transform", finite=True)
    with np.errstate(over="ignore"):
        return np.ascontiguousarray(np.linalg.inv(T)[:3, :].reshape(12).astype(np.float32))


class Volume:
    """``Volume(params, device)``: the five planes of ``regnet_tsdf_*`` in one tensor, reset.  ``D`` (N) float32, ``W`` (N) int32
    and ``C`` (3, N) float32 are views of it, N = nx ny nz, voxel (ix, iy, iz) at ``(iz ny + iy) nx + ix``."""

    def __init__(self, params=None, device="cuda:0"):
        import torch
        self.params = TsdfParams() if params is None else TsdfParams.coerce(params)
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("Volume: the device must be a GPU (no CPU path)")
        nx, ny, nz = self.params.dims
        n = nx * ny * nz
        if int(_L.regnet_tsdf_bytes(nx, ny, nz)) != 20 * n:
            _lib.check(-3, "Volume (at most 2^28 voxels)")
        self.data = torch.empty((5 * n,), dtype=torch.float32, device=self.device)
        self.D, self.W, self.C = self.data[:n], self.data[n:2 * n].view(torch.int32), self.data[2 * n:].view(3, n)
        self.origin = np.ascontiguousarray(np.asarray(self.params.origin, dtype=np.float64).astype(np.float32))
        self.reset()

    @property
    def bytes(self):
        """Bytes of the volume on the device: 20 per voxel."""
        return int(self.data.numel()) * 4

    def reset(self, stream=None):
        """D = 1, W = 0, C = 0.  No host read."""
        import torch
        nx, ny, nz = self.params.dims
        with torch.cuda.device(self.device), stream_scope(stream):
            _lib.call("regnet_tsdf_reset", self.data, self.data.data_ptr(), nx, ny, nz,
                      stream=None if stream is None else stream.cuda_stream)
            record_streams(stream, self.data)      # written on `stream`: keep the allocation alive for it

    def integrate(self, view, pose=None, depth_params=None, stream=None):
        """One view into the volume.  ``view``: a ``depth_frame.DepthFrame`` (it goes through ``to_cloud`` with ``depth_params``)
        or ``(xyz, rgb, width, height, Intrinsics)`` already on the device: the organised cloud (height width, 3) float32 in the
        camera's frame, its colours or None; ``pose``: the camera-to-common 4x4 or None (identity).  -> ``counts`` (4) int32 on
        the device: the voxels this call updated, that were not in view, whose pixel had no depth, and that lay more than
        ``trunc`` behind the surface.  No host read."""
        import torch
        p = self.params
        if isinstance(view, depth_frame.DepthFrame):
            xyz, rgb = depth_frame.to_cloud(view, depth_params, device=self.device, stream=stream)
            height, width = int(view.depth.shape[0]), int(view.depth.shape[1])
            k = view.intrinsics
        else:
            if not isinstance(view, (tuple, list)) or len(view) != 5:
                raise TypeError("integrate takes a DepthFrame or (xyz, rgb, width, height, Intrinsics)")
            xyz, rgb, width, height, k = view
            width, height, k = int(width), int(height), depth_frame.Intrinsics.coerce(k)
        xyz = require_cuda("xyz", xyz, torch.float32, 3, error=TypeError).contiguous()
        if rgb is not None:
            rgb = require_cuda("rgb", rgb, torch.float32, 3, error=TypeError).contiguous()
            if rgb.shape[0] != xyz.shape[0]:
                raise ValueError("integrate: xyz and rgb must have the same rows")
        if xyz.device != self.device or (rgb is not None and rgb.device != self.device):
            raise RuntimeError("integrate: the view is on %s, the volume on %s" % (xyz.device, self.device))
        if width < 1 or height < 1 or int(xyz.shape[0]) != width * height:
            raise ValueError("integrate: xyz must be the organised cloud of its %d x %d frame" % (width, height))
        with np.errstate(over="ignore"):
            intrinsics = np.ascontiguousarray(np.asarray(k.astuple(), dtype=np.float64).astype(np.float32))
        to_camera = camera_from_common(pose)
        nx, ny, nz = p.dims
        with torch.cuda.device(self.device), stream_scope(stream):
            counts = torch.empty((4,), dtype=torch.int32, device=self.device)
            _lib.call("regnet_tsdf_integrate_f32", self.data, self.data.data_ptr(), nx, ny, nz, self.origin.ctypes.data,
                      float(p.voxel), float(p.trunc), int(p.max_weight), xyz.data_ptr(), None if rgb is None else rgb.data_ptr(),
                      width, height, intrinsics.ctypes.data, to_camera.ctypes.data, counts.data_ptr(),
                      stream=None if stream is None else stream.cuda_stream)
            record_streams(stream, xyz, rgb, self.data)
        return counts

    def extract(self, stream=None, out=None):
        """The surface of the volume as it stands -> ``Surface``.  ``out``: ``(xyz, rgb, normal, weight, num)`` contiguous device
        tensors of the result's shapes to write into instead of new ones.  Two passes with an exclusive ``torch.cumsum`` of the
        per-workgroup counts between them; no host read."""
        import torch
        p = self.params
        nx, ny, nz = p.dims
        mp = int(p.max_points)
        dev = self.device
        raw = None if stream is None else stream.cuda_stream
        shapes = (((mp, 3), torch.float32), ((mp, 3), torch.float32), ((mp, 3), torch.float32), ((mp,), torch.int32),
                  ((4,), torch.int32))
        with torch.cuda.device(dev), stream_scope(stream):
            if out is None:
                out = tuple(torch.empty(shape, dtype=dtype, device=dev) for shape, dtype in shapes)
            for t, (shape, dtype) in zip(out, shapes):
                if not (t.is_cuda and t.device == dev and tuple(t.shape) == shape and t.dtype == dtype and t.is_contiguous()):
                    raise ValueError("extract: out must be contiguous device tensors (mp,3) x 3 float32, (mp) and (4) int32")
            xyz, rgb, normal, weight, num = out
            block_counts = torch.empty((int(_L.regnet_tsdf_blocks(nx, ny, nz)),), dtype=torch.int32, device=dev)
            _lib.call("regnet_tsdf_count", self.data, self.data.data_ptr(), nx, ny, nz, int(p.min_weight), block_counts.data_ptr(),
                      num.data_ptr(), stream=raw)
            block_base = torch.cumsum(block_counts, 0, dtype=torch.int32) - block_counts      # exclusive; at most 3 * 2^28 in all
            _lib.call("regnet_tsdf_emit_f32", self.data, self.data.data_ptr(), nx, ny, nz, self.origin.ctypes.data, float(p.voxel),
                      int(p.min_weight), block_counts.data_ptr(), block_base.data_ptr(), mp, xyz.data_ptr(), rgb.data_ptr(),
                      normal.data_ptr(), weight.data_ptr(), num.data_ptr(), stream=raw)
            record_streams(stream, self.data)
        return Surface(xyz, rgb, normal, weight, num, p)


def fuse_volume(multiview, depth_params=None, tsdf_params=None, device="cuda:0", stream=None, register=None, volume=None):
    """``depth_frame.to_cloud`` for every frame of ``multiview`` (a ``fusion.MultiView``), then reset, ``integrate`` in view order
    and ``extract`` -> ``Surface``, which carries ``counts`` (views,4) int32 on the device and ``volume``.  No host read.  With
    ``register`` (a ``registration.IcpParams`` or a dict of its fields) the poses go through ``fusion.refine_poses`` first -- its
    reads are then made -- and the result carries them: ``Surface.poses`` (V,4,4) float64 and ``Surface.register``, the (V,5)
    report.  ``volume``: a ``Volume`` to reuse instead of allocating one (its parameters then hold, and it is reset)."""
    import torch
    from . import fusion
    if not isinstance(multiview, fusion.MultiView):
        raise TypeError("fuse_volume takes a MultiView")
    if volume is None:
        volume = Volume(tsdf_params, device)
    device = volume.device
    clouds = [depth_frame.to_cloud(frame, depth_params, device=device, stream=stream) for frame in multiview.frames]
    poses, report = multiview.poses, None
    if register is not None:
        from . import registration
        poses, report = fusion.refine_poses(clouds, multiview.poses, registration.IcpParams.coerce(register), stream=stream,
                                            frames=multiview.frames)
    volume.reset(stream=stream)
    counts = []
    for (xyz, rgb), frame, pose in zip(clouds, multiview.frames, poses):
        height, width = int(frame.depth.shape[0]), int(frame.depth.shape[1])
        counts.append(volume.integrate((xyz, rgb, width, height, frame.intrinsics), pose, stream=stream))
    surface = volume.extract(stream=stream)
    with stream_scope(stream):
        surface.counts = torch.stack(counts)
    surface.volume = volume
    if report is not None:
        surface.poses, surface.register = np.stack(poses), report
    return surface
