"""Several depth cameras, one cloud (csrc/fuse.hip): a voxel-grid merge of up to 8 posed clouds on the device.

``voxel_merge`` takes the ``(xyz, rgb)`` pairs ``depth_frame.to_cloud`` gives, one per camera, and each camera's pose in a common
frame, and returns one point per occupied voxel: the centroid of the voxel's points and colours, in ascending order of the voxel
key.  Where two views overlap the merged cloud is as dense as where one view looks, which a concatenation is not -- and the
random choice and the furthest point sampling behind ``ingest.ingest_frame`` both follow the density.  A voxel accumulates
integers only (24-bit fractions of the voxel edge, 8-bit colours), so the result does not depend on the order in which the
atomics land: it is bitwise reproducible, and ``tests/fuse_reference.py`` restates it in numpy exactly (include/regnet_hip.h,
DESIGN.md par. 5).  Three launches of the kernels with one ``torch.sort`` of the kept keys between the last two; no host read,
no synchronisation.  GPU only: there is no CPU path.

``MultiView`` holds the ``DepthFrame`` of every camera and its pose; ``fuse_frames`` deprojects each and merges them, and
``GraspDetector.detect`` accepts one where it accepts a ``DepthFrame``.  ``save_npz`` / ``load_npz`` keep a ``MultiView`` in one
``.npz`` with a ``views`` entry, a format of its own next to ``depth_frame``'s.

The merge is only as good as the poses: ``refine_poses`` corrects them first, registering every view onto one reference view by
point-to-plane ICP on the device (``registration.icp``, csrc/icp.hip), with one host read for all views; ``fuse_frames`` runs it
when given ``register``.  The pairs are found by a grid search or, with ``association="projective"``, by a lookup in the reference
view's depth image.
"""
import warnings
from dataclasses import dataclass
from typing import Any, List, Tuple

import numpy as np

from . import _lib, depth_frame
from ._frame_util import MAX_FRAME_POINTS, ParamsBase, matrix4, record_streams, require_cuda, stream_scope, to_device

_L = _lib.lib

MAX_VIEWS = 8
MAX_VOXELS = MAX_FRAME_POINTS       # regnet_fuse_*'s documented limit
COORD_LIMIT = 1 << 20               # voxel coordinates lie in [-2^20, 2^20)


@dataclass(frozen=True)
class FuseParams(ParamsBase):
    """``voxel``: the voxel edge [m]; ``origin``: a corner of voxel (0, 0, 0) in the common frame; ``max_voxels``: the rows of the
    result, at most 2^21 -- a merge that occupies more sets the overflow flag; ``min_count``: voxels with fewer points are dropped
    (2 and more remove isolated points, and points only one camera sees once where two overlap pixel for pixel).

    The 2 mm default is a choice -- about the spacing of the points of a 640 x 480 frame at 1 m -- and not a measurement on real
    cameras.  A voxel below the point spacing makes the merge a pure transform-and-sort: every voxel holds one point, which comes
    out as it went in."""
    WORD, NONE_IS_DEFAULT = "fuse", True
    voxel: float = 0.002
    origin: Tuple[float, float, float] = (0.0, 0.0, 0.0)
    max_voxels: int = 1 << 20
    min_count: int = 1

    def __post_init__(self):
        if not (float(self.voxel) > 0.0 and np.isfinite(self.voxel)):
            raise ValueError("fuse: voxel must be positive and finite")
        origin = tuple(float(v) for v in self.origin)
        if len(origin) != 3 or not all(np.isfinite(v) for v in origin):
            raise ValueError("fuse: origin must be three finite values")
        object.__setattr__(self, "origin", origin)
        if int(self.max_voxels) != self.max_voxels or not 1 <= self.max_voxels <= MAX_VOXELS:
            raise ValueError("fuse: max_voxels must be in 1..2^21")
        if int(self.min_count) != self.min_count or self.min_count < 1:
            raise ValueError("fuse: min_count must be at least 1")


class Fused:
    """``voxel_merge``'s result, all on the device and ``max_voxels`` rows long: ``xyz`` / ``rgb`` (max_voxels,3) float32, NaN / 0
    beyond the ``K`` merged points; ``count`` (points of the voxel), ``views`` (bit v: view v contributed) and ``first`` (the
    smallest global row of the voxel) int32, -1 beyond ``K``; ``num`` (4) int32 = (K, rows merged, rows dropped as non-finite or
    out of range, overflow)."""

    def __init__(self, xyz, rgb, count, views, first, num, params, num_views):
        self.xyz, self.rgb, self.count, self.views, self.first, self.num = xyz, rgb, count, views, first, num
        self.params, self.num_views = params, int(num_views)
        self.poses = self.register = None       # set by fuse_frames(register=...): the refined poses and refine_poses' report

    def check(self):
        """The one blocking read, 16 bytes -> (K, rows merged, rows dropped).  Raises ``ValueError`` when the merge overflowed:
        the rows are then a merge of only a part of the input."""
        k, merged, dropped, overflow = (int(v) for v in self.num.cpu())
        if overflow:
            raise ValueError("fusion: the views occupy more than max_voxels = %d voxels of %g m; raise max_voxels (at most 2^21) "
                             "or the voxel size" % (self.params.max_voxels, self.params.voxel))
        return k, merged, dropped

    def cloud(self):
        """The ``(xyz, rgb)`` pair ``ingest.ingest_frame`` and ``table_plane.calibrate`` take as they are: the rows beyond ``K``
        are NaN rows, which both treat as absent, so nothing is read between fusion and ingest."""
        return self.xyz, self.rgb

    def per_view(self):
        """(num_views,) int64 on the device: the merged points each view contributed to."""
        import torch
        bits = torch.arange(self.num_views, device=self.views.device, dtype=torch.int32)
        seen = (self.views.clamp(min=0)[:, None] >> bits[None, :]) & 1
        return seen.sum(dim=0)


def table_slots(max_voxels):
    """Slots of the hash table of a merge of at most ``max_voxels`` voxels: 2 * next_pow2(max_voxels); -1 outside [1, 2^21]."""
    return int(_L.regnet_fuse_table_slots(int(max_voxels)))


def workspace_bytes(max_voxels):
    """Bytes of scratch the three stages share; -1 for ``max_voxels`` outside [1, 2^21]."""
    return int(_L.regnet_fuse_workspace_bytes(int(max_voxels)))


def pose12(pose):
    """A row-major 4x4 (None: identity) -> its first three rows as 12 float32, each entry rounded once from float64."""
    T = np.eye(4) if pose is None else matrix4(pose, "a pose must be a 4x4 camera-to-common transform")
    with np.errstate(over="ignore"):
        return np.ascontiguousarray(T[:3, :].reshape(12).astype(np.float32))


def _cloud(v, pair, dev):
    import torch
    what = "cloud %d: " % v
    if not isinstance(pair, (tuple, list)) or len(pair) != 2:
        raise TypeError("cloud %d must be an (xyz, rgb) pair" % v)
    out = []
    for name, t in zip(("xyz", "rgb"), pair):
        if t is None and name == "rgb":
            out.append(None)
            continue
        require_cuda(what + name, t, torch.float32, 3, error=TypeError)
        if dev is not None and t.device != dev:
            raise RuntimeError("cloud %d: %s is on %s, the first cloud on %s" % (v, name, t.device, dev))
        out.append(t.contiguous())
    if out[1] is not None and out[1].shape[0] != out[0].shape[0]:
        raise ValueError("cloud %d: xyz and rgb must have the same rows" % v)
    return out


def voxel_merge(clouds, poses=None, params=None, stream=None, out=None):
    """``clouds``: a list of 1..8 ``(xyz, rgb)`` pairs of (n_v, 3) float32 device tensors (``rgb`` None for every one of them: the
    colours of the result are 0); ``poses``: per cloud a row-major 4x4 camera-to-common transform or None for identity (None:
    all identity); ``params``: a ``FuseParams``, a dict of its fields or None; ``stream``: a ``torch.cuda.Stream`` (default: the
    current one); ``out``: ``(xyz, rgb, count, views, first, num)`` contiguous device tensors of the result's shapes to write into
    instead of new ones -> ``Fused``.  Rows with a non-finite coordinate (``to_cloud``'s removed pixels) are skipped.  No host read."""
    import torch
    params = FuseParams.coerce(params)
    clouds = list(clouds)
    if not 1 <= len(clouds) <= MAX_VIEWS:
        raise ValueError("voxel_merge takes 1 to %d clouds, not %d" % (MAX_VIEWS, len(clouds)))
    poses = [None] * len(clouds) if poses is None else list(poses)
    if len(poses) != len(clouds):
        raise ValueError("voxel_merge: one pose per cloud")
    pose_rows = [pose12(p) for p in poses]
    dev, pairs = None, []
    for v, pair in enumerate(clouds):
        xyz, rgb = _cloud(v, pair, dev)
        dev = xyz.device
        pairs.append((xyz, rgb))
    if len({rgb is None for _, rgb in pairs}) != 1:
        raise ValueError("voxel_merge: either every cloud has colours or none has")
    if sum(int(xyz.shape[0]) for xyz, _ in pairs) >= 1 << 31:
        _lib.check(-3, "voxel_merge (fewer than 2^31 rows in all)")
    mv = int(params.max_voxels)
    origin = np.ascontiguousarray(np.asarray(params.origin, dtype=np.float64).astype(np.float32))
    voxel = float(params.voxel)
    raw = None if stream is None else stream.cuda_stream
    with torch.cuda.device(dev), stream_scope(stream):
        ws = torch.empty((workspace_bytes(mv),), dtype=torch.uint8, device=dev)
        kept_keys = torch.empty((mv,), dtype=torch.int64, device=dev)
        shapes = (((mv, 3), torch.float32), ((mv, 3), torch.float32), ((mv,), torch.int32), ((mv,), torch.int32),
                  ((mv,), torch.int32), ((4,), torch.int32))
        if out is None:
            out = tuple(torch.empty(shape, dtype=dtype, device=dev) for shape, dtype in shapes)
        for t, (shape, dtype) in zip(out, shapes):
            if not (t.is_cuda and t.device == dev and tuple(t.shape) == shape and t.dtype == dtype and t.is_contiguous()):
                raise ValueError("voxel_merge: out must be contiguous device tensors (mv,3) (mv,3) float32, (mv) x 3 and (4) int32")
        xyz_out, rgb_out, count, views, first, num = out
        offset = 0
        for v, (xyz, rgb) in enumerate(pairs):
            n = int(xyz.shape[0])
            _lib.call("regnet_fuse_accumulate_f32", ws, xyz.data_ptr(), None if rgb is None else rgb.data_ptr(), n, v, offset,
                      pose_rows[v].ctypes.data, origin.ctypes.data, voxel, mv, 1 if v == 0 else 0, ws.data_ptr(), stream=raw)
            offset += n
        _lib.call("regnet_fuse_finalise_f32", ws, mv, int(params.min_count), kept_keys.data_ptr(), ws.data_ptr(), stream=raw)
        order = torch.sort(kept_keys).indices              # the output order: ascending key (the keys are distinct)
        _lib.call("regnet_fuse_emit_f32", ws, order.data_ptr(), origin.ctypes.data, voxel, mv, xyz_out.data_ptr(),
                  rgb_out.data_ptr(), count.data_ptr(), views.data_ptr(), first.data_ptr(), num.data_ptr(), ws.data_ptr(),
                  stream=raw)
        if stream is not None:                              # the inputs are read on `stream`: keep them alive for it
            record_streams(stream, *(t for pair in pairs for t in pair))
    return Fused(xyz_out, rgb_out, count, views, first, num, params, len(pairs))


@dataclass
class MultiView:
    """The frames of 1..8 depth cameras and their poses: ``frames`` a list of ``depth_frame.DepthFrame``, ``poses`` per frame the
    row-major 4x4 transform from that camera to the common frame -- usually the first camera's, whose pose may then be None."""
    frames: List[Any]
    poses: List[Any] = None

    def __post_init__(self):
        self.frames = list(self.frames)
        if not 1 <= len(self.frames) <= MAX_VIEWS:
            raise ValueError("MultiView: 1 to %d frames" % MAX_VIEWS)
        for frame in self.frames:
            if not isinstance(frame, depth_frame.DepthFrame):
                raise TypeError("MultiView: every frame must be a DepthFrame")
        poses = [None] * len(self.frames) if self.poses is None else list(self.poses)
        if len(poses) != len(self.frames):
            raise ValueError("MultiView: one pose per frame")
        self.poses = [None if p is None else np.array(pose_matrix(p)) for p in poses]


def pose_matrix(pose):
    """A pose as a (4, 4) float64 array; anything else is a ValueError."""
    return matrix4(pose, "a pose must be a finite 4x4 camera-to-common transform", finite=True)


def transform_cloud(xyz, pose):
    """``xyz`` (n,3) float32 on the device taken through ``pose`` (4x4 or None) in ``voxel_merge``'s float32 arithmetic:
    ``pose12``'s entries, ((r0 x + r1 y) + r2 z) + r3 per coordinate, every operation rounded on its own."""
    import torch
    r = [float(v) for v in pose12(pose)]
    x, y, z = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    return torch.stack([((x * r[4 * k] + y * r[4 * k + 1]) + z * r[4 * k + 2]) + r[4 * k + 3] for k in range(3)], dim=1)


def _frame_geometry(v, frame):
    """A view's ``DepthFrame``, or its ``(width, height, Intrinsics)`` -> (width, height, Intrinsics)."""
    if isinstance(frame, depth_frame.DepthFrame):
        if not hasattr(frame.depth, "shape") or len(frame.depth.shape) != 2:
            raise ValueError("refine_poses: the depth image of view %d must be (H, W)" % v)
        return int(frame.depth.shape[1]), int(frame.depth.shape[0]), frame.intrinsics
    if not isinstance(frame, (tuple, list)) or len(frame) != 3:
        raise TypeError("refine_poses: frames[%d] must be a DepthFrame or (width, height, Intrinsics)" % v)
    return int(frame[0]), int(frame[1]), depth_frame.Intrinsics.coerce(frame[2])


def refine_poses(clouds, poses, params=None, reference=0, stream=None, frames=None):
    """Correct the poses of several cameras against one of them before ``voxel_merge`` (``registration.icp``, csrc/icp.hip).
    ``clouds``: per view ``xyz`` (n_v,3) float32 on the device in ITS CAMERA's frame, or the ``(xyz, rgb)`` pair ``voxel_merge``
    takes; ``poses``: per view the 4x4 camera-to-common transform or None (identity); ``params``: a ``registration.IcpParams``,
    a dict of its fields or None; ``reference``: the view every other one is registered onto -- its cloud, taken into the common
    frame by its own pose, is the target, its normals estimated facing its camera.  Every registration starts from the view's
    given pose; all are enqueued, then ONE host read fetches every state block.
    -> (poses, report): a list of (4,4) float64 arrays and (V,5) float64 = (status, iterations, pairs, rms first, rms last) per
    view; the reference's row is (-1, 0, 0, 0, 0).  A view that ended TOO_FEW or DEGENERATE keeps its given pose.

    With ``params.association == "projective"`` the pairs are looked up in the reference's depth image and ``frames`` is needed:
    per view its ``DepthFrame``, or ``(width, height, Intrinsics)``, whose organised cloud ``clouds[v]`` is.  The reference's cloud
    then stays in its own camera's frame and is not compacted (no host read before the one at the end); view v starts from
    inv(P_ref) P_v, a float64 product on the host, and ends as P_ref T_v."""
    import torch
    from . import registration
    params = registration.IcpParams.coerce(params) or registration.IcpParams()
    clouds = [c[0] if isinstance(c, (tuple, list)) else c for c in clouds]
    if not 1 <= len(clouds) <= MAX_VIEWS:
        raise ValueError("refine_poses takes 1 to %d clouds, not %d" % (MAX_VIEWS, len(clouds)))
    poses = [None] * len(clouds) if poses is None else list(poses)
    if len(poses) != len(clouds):
        raise ValueError("refine_poses: one pose per cloud")
    if int(reference) != reference or not 0 <= reference < len(clouds):
        raise ValueError("refine_poses: reference must name one of the %d views" % len(clouds))
    given = [np.eye(4) if p is None else np.array(pose_matrix(p)) for p in poses]
    for v, xyz in enumerate(clouds):
        require_cuda("cloud %d" % v, xyz, torch.float32, 3, error=TypeError)
    report = np.zeros((len(clouds), 5), dtype=np.float64)
    report[reference, 0] = -1.0
    others = [v for v in range(len(clouds)) if v != reference]
    if not others:
        return given, report
    dev = clouds[reference].device
    if params.association == "projective":
        if frames is None:
            raise ValueError("refine_poses: association='projective' needs frames, the depth frames (or (width, height, "
                             "Intrinsics)) the clouds were made from")
        frames = list(frames)
        if len(frames) != len(clouds):
            raise ValueError("refine_poses: one frame per cloud")
        shapes = [_frame_geometry(v, frame) for v, frame in enumerate(frames)]
        for v, (w, h, _) in enumerate(shapes):
            if int(clouds[v].shape[0]) != w * h:
                raise ValueError("refine_poses: cloud %d is not the organised cloud of its %d x %d frame" % (v, w, h))
        to_reference = np.linalg.inv(given[reference])
        with torch.cuda.device(dev), stream_scope(stream):
            w, h, k = shapes[reference]
            target = registration.prepare_projective_target(clouds[reference], w, h, k, params, stream=stream,
                                                            max_source=max(int(clouds[v].shape[0]) for v in others))
            starts = [to_reference @ given[v] for v in others]
            blocks = to_device(np.stack([registration.initial_state(start, params) for start in starts]), dev)
            for row, v in enumerate(others):
                registration.icp(clouds[v], target, starts[row], params, stream=stream, state=blocks[row],
                                 source_shape=shapes[v][:2])
            raw = blocks.cpu().numpy()                               # the one host read, 1152 bytes per registered view
        refined = list(given)
        for row, v in enumerate(others):
            decoded = registration.decode_state(raw[row])
            report[v] = registration.report_row(decoded)
            if decoded["status"] not in (registration.TOO_FEW, registration.DEGENERATE):
                refined[v] = given[reference] @ decoded["pose"]
        return refined, report
    with torch.cuda.device(dev), stream_scope(stream):
        target = registration.prepare_target(transform_cloud(clouds[reference], given[reference]), params,
                                             target_camera=tuple(given[reference][:3, 3]),
                                             max_source=max(int(clouds[v].shape[0]) for v in others), stream=stream)
        blocks = to_device(np.stack([registration.initial_state(given[v], params) for v in others]), dev)
        for row, v in enumerate(others):
            registration.icp(clouds[v], target, given[v], params, stream=stream, state=blocks[row])
        raw = blocks.cpu().numpy()                                   # the one host read, 1152 bytes per registered view
    refined = list(given)
    for row, v in enumerate(others):
        decoded = registration.decode_state(raw[row])
        report[v] = registration.report_row(decoded)
        if decoded["status"] not in (registration.TOO_FEW, registration.DEGENERATE):
            refined[v] = decoded["pose"]
    return refined, report


def fuse_frames(multiview, depth_params=None, fuse_params=None, device="cuda:0", stream=None, register=None):
    """``depth_frame.to_cloud`` for every frame of ``multiview``, then ``voxel_merge`` -> ``Fused``.  No host read.  With
    ``register`` (a ``registration.IcpParams`` or a dict of its fields) the poses go through ``refine_poses`` first -- its reads
    are then made -- and the result carries them: ``Fused.poses`` (V,4,4) float64 and ``Fused.register``, the (V,5) report."""
    if not isinstance(multiview, MultiView):
        raise TypeError("fuse_frames takes a MultiView")
    clouds = [depth_frame.to_cloud(frame, depth_params, device=device, stream=stream) for frame in multiview.frames]
    if register is None:
        return voxel_merge(clouds, multiview.poses, fuse_params, stream=stream)
    from . import registration
    register = registration.IcpParams.coerce(register)
    if register.stride > 1:                    # the cloud is organised row by row; the width is read off the shape, host or device
        widths = [(v, int(frame.depth.shape[-1])) for v, frame in enumerate(multiview.frames) if hasattr(frame.depth, "shape")]
        whole = [(v, w) for v, w in widths if w % int(register.stride) == 0]
        if whole:
            warnings.warn("register: a stride of %d divides the width of view%s %s (%s pixels) and visits whole pixel columns only; "
                          "take one that does not" % (register.stride, "" if len(whole) == 1 else "s",
                                                      ", ".join(str(v) for v, _ in whole), ", ".join(str(w) for _, w in whole)))
    poses, report = refine_poses(clouds, multiview.poses, register, stream=stream, frames=multiview.frames)
    fused = voxel_merge(clouds, poses, fuse_params, stream=stream)
    fused.poses, fused.register = np.stack(poses), report
    return fused


_VIEW_KEYS = ("depth", "intrinsics", "pose", "color", "color_intrinsics", "depth_to_color", "depth_scale")


def is_multiview_npz(path):
    """Whether the ``.npz`` at ``path`` has a ``views`` entry (then ``load_npz`` here reads it, else ``depth_frame``'s)."""
    with np.load(path, allow_pickle=False) as data:
        return "views" in data.files


def save_npz(path, multiview):
    """Write ``multiview`` as one ``.npz``: ``views`` (the count) and per view ``view{v}_pose`` (4,4) and
    ``depth_frame.frame_items``' entries behind ``view{v}_``."""
    items = {"views": np.int64(len(multiview.frames))}
    for v, (frame, pose) in enumerate(zip(multiview.frames, multiview.poses)):
        items.update(depth_frame.frame_items(frame, "view%d_" % v))
        items["view%d_pose" % v] = np.eye(4) if pose is None else pose_matrix(pose)
    with open(path, "wb") as f:
        np.savez(f, **items)


def load_npz(path):
    """Read a ``.npz`` written by ``save_npz`` (or by anything that uses its entries) -> ``MultiView``.  Unknown entries, a
    missing depth image, intrinsics or pose are a ``ValueError``."""
    what = "multi-view frame %s" % path
    with np.load(path, allow_pickle=False) as data:
        if "views" not in data.files:
            raise ValueError("%s: no 'views' entry" % what)
        count = int(data["views"])
        if not 1 <= count <= MAX_VIEWS:
            raise ValueError("%s: views must be 1..%d" % (what, MAX_VIEWS))
        depth_frame.check_npz_entries(data, {"views"} | {"view%d_%s" % (v, key) for v in range(count) for key in _VIEW_KEYS}, what)
        frames = [depth_frame.frame_from_items(data, "view%d_" % v, what, ("depth", "intrinsics", "pose")) for v in range(count)]
        return MultiView(frames, [pose_matrix(data["view%d_pose" % v]) for v in range(count)])
