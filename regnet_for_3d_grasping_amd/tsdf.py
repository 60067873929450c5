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

``Volume.raycast`` renders the volume from any pose: per pixel of a virtual pinhole camera the first zero crossing along its
ray, with the gradient's normal and the colour there -- a denoised depth and normal image of the fused model (``ModelView``),
laid out as ``registration.ProjectiveTarget`` takes it.  ``Tracker`` closes the loop for a camera whose pose is NOT given (one
on the robot's wrist): every new frame is registered against the model view from the last pose and integrated at the pose
found -- frame-to-model tracking, KinectFusion's third leg.  ``tests/tsdf_raycast_reference.py`` restates both.  With
``TrackParams.levels`` / ``smooth`` the registration descends a pyramid of the frame's (optionally bilateral-filtered) depth
image coarse to fine on one state block (``depth_frame.pyramid``, ``registration.continue_state``;
``tests/depth_pyramid_reference.py``); off by default.

``Volume.extract_mesh`` returns the surface as a triangle mesh (csrc/tsdf_mesh.hip): the rows of ``extract`` are the vertices,
and marching cubes over the cells whose eight corners were observed adds the index buffer, in cell order with no sort -- integer
work only, so ``tests/tsdf_mesh_reference.py`` restates it with plain loops.  ``Mesh.save_ply`` writes it for a viewer, a
simulator or a planner's collision world.  ``Mesh.simplify`` merges its vertices per cell of a coarse grid and de-duplicates the
index buffer (csrc/mesh_simplify.hip, vertex clustering): integer accumulation in the grid's order, so
``tests/mesh_simplify_reference.py`` restates it bit for bit too.
"""
from dataclasses import dataclass, replace
import math
from typing import Optional, Tuple

import numpy as np

from . import _lib, depth_frame
from ._frame_util import MAX_FRAME_POINTS, ParamsBase, matrix4, record_streams, require_cuda, stream_scope, to_device

_L = _lib.lib

MAX_VOLUME_VOXELS = 1 << 28         # regnet_tsdf_*'s documented limits
MAX_POINTS = MAX_FRAME_POINTS
MAX_TRIANGLES = 1 << 22             # regnet_tsdf_mesh_emit's documented limit
BLOCK = 256                         # voxels per workgroup of the two extraction passes
MAX_SIMPLIFY_CELLS = 1 << 21        # regnet_mesh_simplify_f32's documented limit on the coarse grid
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


class Mesh:
    """``Volume.extract_mesh``'s result, on the device: ``surface``, the ``Surface`` of the same call and volume state, whose rows
    are the vertices; ``triangles`` (max_triangles,3) int32, rows of ``surface`` per triangle in ascending order of the cell (the
    linear index of its low corner voxel), -1 beyond the ``Kt`` rows; ``num_triangles`` (4) int32 = (Kt, triangles in all, dropped,
    overflow).  A triangle one of whose vertices the surface dropped (it overflowed ``max_points``) is (-1, -1, -1) in its place
    and counted in ``dropped``.  The right-hand-rule normal of a triangle points where the surface's normals point, out of the
    solid.  Where a voxel's distance is exactly 0 up to three vertices coincide and the triangles between them have no area; they
    are kept, so the mesh stays closed.  A cell with a corner that was not observed ``min_weight`` times has no triangles: the mesh
    is open along the border of observed space."""

    def __init__(self, surface, triangles, num_triangles, max_triangles, volume=None):
        self.surface, self.triangles, self.num_triangles, self.max_triangles = surface, triangles, num_triangles, int(max_triangles)
        self.volume = volume                    # the Volume it was extracted from: where ``simplify`` keeps its buffers
        self.simplify_buffers = {}              # ... and where it keeps them for a mesh without one

    def check(self):
        """Two blocking reads of 16 bytes -> (vertices K, triangles Kt).  Raises ``ValueError`` when the surface or the triangles
        overflowed, or a triangle was dropped."""
        k = self.surface.check()[0]
        kt, total, dropped, overflow = (int(v) for v in self.num_triangles.cpu())
        if overflow:
            raise ValueError("tsdf: the mesh has %d triangles, more than max_triangles = %d; raise max_triangles (at most 2^22) or "
                             "the voxel size" % (total, self.max_triangles))
        if dropped:
            raise ValueError("tsdf: %d triangles lost a vertex to the surface's max_points" % dropped)
        return k, kt

    def to_host(self):
        """-> ``(vertices (K,3) float32, normals (K,3) float32, colours (K,3) float32, triangles (M,3) int32)`` as numpy arrays,
        compacted: the K surface rows, and the triangles without the dropped ones.  Blocking reads; raises nothing."""
        s = self.surface
        k = int(s.num[0].item())
        kt = int(self.num_triangles[0].item())
        tri = self.triangles[:kt].cpu().numpy()
        return (s.xyz[:k].cpu().numpy(), s.normal[:k].cpu().numpy(), s.rgb[:k].cpu().numpy(),
                np.ascontiguousarray(tri[tri[:, 0] >= 0]))

    def save_ply(self, path):
        """Writes ``to_host()`` as a binary little-endian PLY: per vertex x y z nx ny nz float32 and red green blue uint8 (the
        colour times 255, rounded, clipped), per face a uint8 3 and three int32."""
        write_ply(path, *self.to_host())

    def simplify(self, cell=None, factor=4, dedupe=True, max_vertices=None, max_triangles=None, stream=None, out=None):
        """Vertex clustering (csrc/mesh_simplify.hip) -> ``SimplifiedMesh``.  The vertices are merged per cell of a dense grid of
        edge ``cell`` [m] (None: ``factor`` voxels) over the volume's box, ``g_k = ceil(n_k voxel / cell) + 1`` cells per axis from
        the volume's origin, at most 2^21 in all: a cell's vertex is the mean of its vertices (one vertex alone is kept bit for
        bit), with the mean colour and the normalised mean normal.  Triangles with two vertices in one cell leave; with ``dedupe``
        triangles that became equal (as oriented triples) are one, the one of the smallest source row.  The new vertices ascend by
        cell, the triangles by source row: no sort, and the same bytes on every run.  ``max_vertices`` (None: the smaller of the
        surface's rows and the cells) and ``max_triangles`` (None: this mesh's) are the rows of the result; one that has more
        sets its overflow flag.

        The workspace and the outputs are allocated on the first call with these sizes and KEPT on the volume: a second call
        allocates nothing and writes the same tensors, so a result is good until the next such call.  ``out``: a
        ``SimplifiedMesh`` of the same sizes (an earlier result) to write into instead.  Two fills and eight launches; no host
        read.  The mesh is no longer manifold in general (DESIGN.md par. 10)."""
        import torch
        s = self.surface
        p = s.params
        voxel = float(p.voxel)
        cell = float(factor) * voxel if cell is None else float(cell)
        with np.errstate(over="ignore", under="ignore"):
            cell32 = np.float32(cell)
        if not (cell > 0.0 and cell32 > 0.0 and np.isfinite(cell32)):
            raise ValueError("simplify: cell must be positive and finite in float32")
        grid = tuple(int(math.ceil(n * voxel / cell)) + 1 for n in p.dims)
        cells = grid[0] * grid[1] * grid[2]
        if cells > MAX_SIMPLIFY_CELLS:
            raise ValueError("simplify: a grid of %d x %d x %d cells, more than 2^21; raise cell" % grid)
        rows, mt_in = int(s.xyz.shape[0]), int(self.max_triangles)
        mv = min(rows, cells) if max_vertices is None else max_vertices
        mt = mt_in if max_triangles is None else max_triangles
        if int(mv) != mv or not 1 <= mv <= MAX_POINTS:
            raise ValueError("simplify: max_vertices must be in 1..2^21")
        if int(mt) != mt or not 1 <= mt <= MAX_TRIANGLES:
            raise ValueError("simplify: max_triangles must be in 1..2^22")
        mv, mt = int(mv), int(mt)
        dev = s.xyz.device
        origin = np.ascontiguousarray(np.asarray(p.origin, dtype=np.float64).astype(np.float32))
        raw = None if stream is None else stream.cuda_stream
        keeper = self if self.volume is None else self.volume
        kept = keeper.simplify_buffers
        with torch.cuda.device(dev), stream_scope(stream):
            sizes = (cells, mt_in, mv, mt)
            if sizes not in kept:
                workspace = torch.empty((int(_L.regnet_mesh_simplify_workspace_bytes(cells, mt_in)) // 8,), dtype=torch.int64,
                                        device=dev)
                kept[sizes] = (workspace, None if out is not None else SimplifiedMesh.empty(mv, mt, p, dev))
            workspace, result = kept[sizes]
            if out is not None:
                if not (isinstance(out, SimplifiedMesh) and out.sizes() == (mv, mt) and out.triangles.device == dev):
                    raise ValueError("simplify: out must be a SimplifiedMesh of %d vertex and %d triangle rows on %s" % (mv, mt, dev))
                result = out
            elif result is None:
                result = SimplifiedMesh.empty(mv, mt, p, dev)
                kept[sizes] = (workspace, result)
            v = result.surface
            _lib.call("regnet_mesh_simplify_f32", s.xyz, s.xyz.data_ptr(), s.normal.data_ptr(), s.rgb.data_ptr(), rows,
                      s.num.data_ptr(), self.triangles.data_ptr(), mt_in, self.num_triangles.data_ptr(), origin.ctypes.data, cell,
                      grid[0], grid[1], grid[2], 1 if dedupe else 0, mv, mt, workspace.data_ptr(), v.xyz.data_ptr(),
                      v.normal.data_ptr(), v.rgb.data_ptr(), v.weight.data_ptr(), result.triangles.data_ptr(),
                      result.report.data_ptr(), v.num.data_ptr(), stream=raw)
            record_streams(stream, s.xyz, s.normal, s.rgb, s.num, self.triangles, self.num_triangles, workspace, v.xyz, v.normal,
                           v.rgb, v.weight, v.num, result.triangles, result.report)
        result.source, result.volume, result.cell, result.grid, result.dedupe = self, self.volume, cell, grid, bool(dedupe)
        return result


class SimplifiedMesh(Mesh):
    """``Mesh.simplify``'s result, on the device: a ``Mesh`` whose ``surface`` is a ``Surface`` of the NEW vertices -- ``weight``
    the source vertices merged into each, ``num`` (4) int32 = (Kv kept, Kv in all, the source's K, overflow) -- and whose
    ``triangles`` index them; ``num_triangles`` has ``Mesh``'s meaning, so ``check``, ``to_host`` and ``save_ply`` work unchanged.
    ``report`` (12) int32: (Kv kept, Kv in all, vertex overflow, occupied cells, stray vertices, Kt kept, survivors in all,
    dropped, triangle overflow, collapsed, duplicate, stray or absent source triangles); ``num_triangles`` is a view of its words
    5..8.  ``source``: the mesh it was made from; ``cell`` [m], ``grid`` and ``dedupe`` say how."""

    def __init__(self, surface, triangles, report, max_triangles):
        Mesh.__init__(self, surface, triangles, report[5:9], max_triangles)
        self.report = report
        self.source = self.cell = self.grid = self.dedupe = None

    @classmethod
    def empty(cls, max_vertices, max_triangles, params, device):
        """The buffers of a result with these rows; what they hold is undefined until ``Mesh.simplify`` wrote them."""
        import torch
        mv, mt = int(max_vertices), int(max_triangles)
        xyz, rgb, normal = (torch.empty((mv, 3), dtype=torch.float32, device=device) for _ in range(3))
        weight = torch.empty((mv,), dtype=torch.int32, device=device)
        num = torch.empty((4,), dtype=torch.int32, device=device)
        surface = Surface(xyz, rgb, normal, weight, num, replace(params, max_points=mv))
        return cls(surface, torch.empty((mt, 3), dtype=torch.int32, device=device),
                   torch.empty((12,), dtype=torch.int32, device=device), mt)

    def sizes(self):
        """-> (vertex rows, triangle rows)."""
        return int(self.surface.xyz.shape[0]), int(self.triangles.shape[0])


def write_ply(path, vertices, normals, colours, triangles):
    """``Mesh.save_ply`` for host arrays."""
    k, m = int(len(vertices)), int(len(triangles))
    vertex = np.zeros((k,), dtype=[("xyz", "<f4", (3,)), ("n", "<f4", (3,)), ("rgb", "u1", (3,))])
    vertex["xyz"], vertex["n"] = vertices, normals
    with np.errstate(invalid="ignore"):
        vertex["rgb"] = np.clip(np.nan_to_num(np.rint(np.asarray(colours, dtype=np.float64) * 255.0)), 0, 255).astype(np.uint8)
    face = np.zeros((m,), dtype=[("n", "u1"), ("v", "<i4", (3,))])
    face["n"], face["v"] = 3, triangles
    header = ("ply\nformat binary_little_endian 1.0\nelement vertex %d\nproperty float x\nproperty float y\nproperty float z\n"
              "property float nx\nproperty float ny\nproperty float nz\nproperty uchar red\nproperty uchar green\n"
              "property uchar blue\nelement face %d\nproperty list uchar int vertex_indices\nend_header\n" % (k, m))
    with open(path, "wb") as f:
        f.write(header.encode("ascii"))
        f.write(vertex.tobytes())
        f.write(face.tobytes())


NO_SURFACE, BACK_FACE, HIT, HIT_NO_NORMAL = 0, 1, 2, 3   # raycast's status codes, the entries of its counts
MAX_RAY_STEPS = 4096                # regnet_tsdf_raycast_f32's documented limit
FIRST, TRACKED, LOST = "FIRST", "TRACKED", "LOST"
TRACK_STATUS = (FIRST, TRACKED, LOST)                    # a record's ``track_status`` is the index
MAX_LEVELS = 4                      # of the tracking pyramid
LEVEL_ITERATIONS = (10, 5, 4, 4)    # the default steps per level, finest first


@dataclass(frozen=True)
class TrackParams(ParamsBase):
    """What ``GraspDetector(track=...)`` and ``Tracker`` take (a dict with these keys works too).

    The registration is ``registration.icp`` with ``association="projective"`` against the model view; ``max_dist``,
    ``iterations``, ``stride``, ``window``, ``min_pairs``, ``rot_eps``, ``trans_eps``, ``normal_angle``, ``normal_step`` and
    ``normal_jump`` are ``IcpParams``' fields of those names and go to it as they are (the last two make the FRAME's normals,
    which only ``normal_angle`` needs; the model's come from the volume).  ``near``, ``far`` [m]: the depths between which a ray
    is marched; ``step`` [m]: the distance between two samples, None: half the volume's ``trunc``, so a ray cannot step over
    the band in which the distance is known; at most 4096 samples per ray.  ``max_translation`` [m] / ``max_rotation`` [rad]:
    a frame that moved further against the pose it was registered from is LOST; ``min_hit_share``: so is one whose model view
    hit the surface in a smaller share of its pixels.

    Every default is a choice: a frame-to-frame motion of centimetres and a few degrees, the capture range of the pose
    refinement, twenty steps of which a tracked frame needs a handful; rays from 20 cm to 1.5 m, which spans the default volume
    seen from about its first camera.  None is measured on real cameras.

    Coarse to fine.  ``levels`` (1..4): the frame's depth image is halved ``levels - 1`` times (``depth_frame.pyramid``) and the
    registration descends from the coarsest level to the frame's own on ONE state block, the model raycast once per level at the
    level's intrinsics and size.  ``level_iterations``: the steps per level, FINEST FIRST, 64 in all at most; None:
    ``(10, 5, 4, 4)[:levels]`` (with one level ``iterations``, which stays the single-level budget).  ``level_dist_scale``: level
    ``l`` pairs within ``max_dist * level_dist_scale**l``; the pixel ``window`` is the same on every level, so in fine pixels it
    doubles per level.  ``smooth`` (a ``depth_frame.SmoothParams`` or a dict of its fields): the frame's depth goes through the
    bilateral filter before the pyramid -- for the registration only; what is integrated is the frame as it came.  With
    ``levels == 1`` and no ``smooth`` nothing of this runs.  These defaults are choices too."""
    WORD = "track"
    NONE_IS_DEFAULT = True
    max_dist: float = 0.02
    iterations: int = 20
    stride: int = 1
    window: int = 1
    min_pairs: int = 100
    rot_eps: float = 1e-5
    trans_eps: float = 1e-6
    normal_angle: Optional[float] = None
    normal_step: int = 2
    normal_jump: float = 0.02
    near: float = 0.2
    far: float = 1.5
    step: Optional[float] = None
    max_translation: float = 0.05
    max_rotation: float = 0.1
    min_hit_share: float = 0.05
    levels: int = 1
    level_iterations: Optional[Tuple[int, ...]] = None
    level_dist_scale: float = 2.0
    smooth: Optional[depth_frame.SmoothParams] = None

    def __post_init__(self):
        self.icp_params()                                   # (its checks are the registration's)
        if int(self.levels) != self.levels or not 1 <= self.levels <= MAX_LEVELS:
            raise ValueError("track: levels must be in 1..%d" % MAX_LEVELS)
        if self.level_iterations is not None:
            budgets = tuple(self.level_iterations)
            if len(budgets) != self.levels or any(int(b) != b or b < 1 for b in budgets) or sum(budgets) > 64:
                raise ValueError("track: level_iterations must be `levels` positive step counts, finest first, 64 in all at most")
            object.__setattr__(self, "level_iterations", tuple(int(b) for b in budgets))
        if not (float(self.level_dist_scale) > 0.0 and math.isfinite(float(self.level_dist_scale))):
            raise ValueError("track: level_dist_scale must be positive and finite")
        for level in range(1, int(self.levels)):
            self.icp_params(level)                          # (a max_dist that leaves float32's range on a coarse level)
        object.__setattr__(self, "smooth", depth_frame.SmoothParams.coerce(self.smooth))
        check_ray_range(self.near, self.far, self.step, "track")
        for name in ("max_translation", "max_rotation"):
            if not float(getattr(self, name)) > 0.0:        # (a NaN too; inf: no gate)
                raise ValueError("track: %s must be positive" % name)
        if not 0.0 <= float(self.min_hit_share) <= 1.0:
            raise ValueError("track: min_hit_share must be in 0..1")

    def pyramid(self):
        """Whether ``Tracker.track`` takes the coarse-to-fine path: more than one level, or a smoothed frame."""
        return self.levels > 1 or self.smooth is not None

    def budgets(self):
        """The steps enqueued per level, finest first: ``level_iterations``, else ``(10, 5, 4, 4)[:levels]``, and with one
        level ``iterations``."""
        if self.level_iterations is not None:
            return self.level_iterations
        return (int(self.iterations),) if self.levels == 1 else LEVEL_ITERATIONS[:self.levels]

    def icp_params(self, level=None):
        """The ``registration.IcpParams`` of a frame-to-model registration; ``level``: those of that level of the pyramid, its
        own step budget and ``max_dist * level_dist_scale**level``."""
        from . import registration
        if level is not None:
            return registration.IcpParams(max_dist=float(self.max_dist) * float(self.level_dist_scale) ** level,
                                          iterations=self.budgets()[level], stride=self.stride, window=self.window,
                                          min_pairs=self.min_pairs, rot_eps=self.rot_eps, trans_eps=self.trans_eps,
                                          normal_angle=self.normal_angle, normal_step=self.normal_step,
                                          normal_jump=self.normal_jump, association="projective")
        return registration.IcpParams(max_dist=self.max_dist, iterations=self.iterations, stride=self.stride, window=self.window,
                                      min_pairs=self.min_pairs, rot_eps=self.rot_eps, trans_eps=self.trans_eps,
                                      normal_angle=self.normal_angle, normal_step=self.normal_step, normal_jump=self.normal_jump,
                                      association="projective")


def check_ray_range(near, far, step, word):
    """``near`` < ``far``, both and ``step`` (None: not looked at) positive and finite in float32, else a ValueError."""
    for name, value in (("near", near), ("far", far), ("step", step)):
        if value is None and name == "step":
            continue
        with np.errstate(over="ignore", under="ignore"):
            as32 = np.float32(value)
        if not (float(value) > 0.0 and as32 > 0.0 and np.isfinite(as32)):
            raise ValueError("%s: %s must be positive and finite in float32" % (word, name))
    if not float(near) < float(far):
        raise ValueError("%s: near must be below far" % word)


def ray_steps(near, far, step):
    """``ceil((far - near) / step)``, in float64: the samples of a ray."""
    return int(math.ceil((float(far) - float(near)) / float(step)))


class ModelView:
    """``Volume.raycast``'s result, on the device: ``xyz`` / ``normals`` / ``rgb`` (H W, 3) float32 IN THE VIRTUAL CAMERA's frame,
    row ``v W + u`` for pixel (u, v), NaN in ``xyz`` without a hit and in ``normals`` without a normal, ``rgb`` 0 without a hit
    (None when no colour was asked for); ``status`` (H W) uint8: ``NO_SURFACE``, ``BACK_FACE``, ``HIT``, ``HIT_NO_NORMAL``;
    ``counts`` (4) int32, its histogram.  ``width``, ``height``, ``intrinsics`` (an ``Intrinsics``) and ``pose`` (4,4) float64,
    camera-to-common, say which camera."""

    def __init__(self, xyz, normals, rgb, status, counts, width, height, intrinsics, pose):
        self.xyz, self.normals, self.rgb, self.status, self.counts = xyz, normals, rgb, status, counts
        self.width, self.height, self.intrinsics, self.pose = int(width), int(height), intrinsics, pose

    def target(self, icp_params=None, max_source=None, stream=None):
        """The view as the target of a projective registration (``registration.prepare_projective_target`` with the model's
        own normals): nothing is compacted and nothing is read."""
        from . import registration
        return registration.prepare_projective_target(self.xyz, self.width, self.height, self.intrinsics, icp_params,
                                                      target_normals=self.normals, stream=stream,
                                                      max_source=registration.MAX_POINTS if max_source is None else max_source)

    def depth(self):
        """The denoised depth image (H, W) float32 on the device, NaN without a hit: a view of ``xyz``."""
        return self.xyz[:, 2].view(self.height, self.width)


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
        self.mesh_scratch = None                # extract_mesh's row lookup plane, (N) int32: allocated on its first call
        self.simplify_buffers = {}              # Mesh.simplify's (workspace, result) per sizes: allocated on the first call with them
        self.view_plane = None                  # view_gain's bit plane, (N) int32: allocated on its first call
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
        return self._extract(self.params, stream, out)[0]

    def _extract(self, p, stream, out):
        """``extract`` with the parameters ``p`` -> (the ``Surface``, block_counts, block_base)."""
        import torch
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
        return Surface(xyz, rgb, normal, weight, num, p), block_counts, block_base

    def extract_mesh(self, min_weight=None, max_points=None, max_triangles=None, stream=None, out=None, out_mesh=None,
                     simplify=None):
        """The surface of the volume as it stands as a triangle mesh -> ``Mesh``: ``extract`` (with ``min_weight`` / ``max_points``
        in place of the volume's parameters when given; ``out`` goes to it) and, on the same state, marching cubes over the
        cells all of whose corners are usable.  ``out_mesh``: ``(triangles, num_triangles)`` contiguous device tensors of the
        result's shapes to write into.  ``max_triangles``: the rows of the index buffer, at most 2^22; None: twice
        ``max_points`` (a closed surface has about two triangles per vertex), capped there.  Five more launches and one more
        ``torch.cumsum``; no host read.  The row lookup's scratch plane, 4 bytes per voxel, is allocated on the first call and
        kept on the volume.  ``simplify``: a cell edge [m]: -> ``Mesh.simplify(cell=simplify)`` of that mesh, a
        ``SimplifiedMesh`` whose ``source`` is the full one; None: nothing more is launched."""
        import torch
        p = self.params
        if min_weight is not None or max_points is not None:
            p = replace(p, min_weight=p.min_weight if min_weight is None else min_weight,
                        max_points=p.max_points if max_points is None else max_points)
        mt = min(2 * int(p.max_points), MAX_TRIANGLES) if max_triangles is None else max_triangles
        if int(mt) != mt or not 1 <= mt <= MAX_TRIANGLES:
            raise ValueError("extract_mesh: max_triangles must be in 1..2^22")
        mt = int(mt)
        nx, ny, nz = p.dims
        dev = self.device
        raw = None if stream is None else stream.cuda_stream
        surface, block_counts, block_base = self._extract(p, stream, out)
        with torch.cuda.device(dev), stream_scope(stream):
            if self.mesh_scratch is None:
                self.mesh_scratch = torch.empty((int(_L.regnet_tsdf_mesh_scratch_bytes(nx, ny, nz)) // 4,), dtype=torch.int32,
                                                device=dev)
            if out_mesh is None:
                out_mesh = (torch.empty((mt, 3), dtype=torch.int32, device=dev), torch.empty((4,), dtype=torch.int32, device=dev))
            tri, num_tri = out_mesh
            for t, shape in ((tri, (mt, 3)), (num_tri, (4,))):
                if not (t.is_cuda and t.device == dev and tuple(t.shape) == shape and t.dtype == torch.int32 and t.is_contiguous()):
                    raise ValueError("extract_mesh: out_mesh must be contiguous device tensors (max_triangles,3) and (4) int32")
            tri_counts = torch.empty((int(_L.regnet_tsdf_mesh_blocks(nx, ny, nz)),), dtype=torch.int32, device=dev)
            _lib.call("regnet_tsdf_mesh_count", self.data, self.data.data_ptr(), nx, ny, nz, int(p.min_weight), tri_counts.data_ptr(),
                      num_tri.data_ptr(), stream=raw)
            tri_base = torch.cumsum(tri_counts, 0, dtype=torch.int32) - tri_counts      # exclusive; at most 5 * 2^28 in all
            _lib.call("regnet_tsdf_mesh_emit", self.data, self.data.data_ptr(), nx, ny, nz, int(p.min_weight),
                      block_counts.data_ptr(), block_base.data_ptr(), surface.num.data_ptr(), tri_counts.data_ptr(),
                      tri_base.data_ptr(), mt, self.mesh_scratch.data_ptr(), tri.data_ptr(), num_tri.data_ptr(), stream=raw)
            record_streams(stream, self.data, self.mesh_scratch, block_counts, block_base, tri_counts, tri_base, tri, num_tri)
        mesh = Mesh(surface, tri, num_tri, mt, volume=self)
        return mesh if simplify is None else mesh.simplify(cell=simplify, stream=stream)

    def raycast(self, pose, intrinsics, width, height, near=None, far=None, step=None, colour=True, stream=None, out=None,
                clip=True):
        """The model view of the volume as it stands from the virtual pinhole camera at ``pose`` (camera-to-common 4x4, None:
        identity) with ``intrinsics`` (an ``Intrinsics`` or (fx, fy, cx, cy)) and ``width`` x ``height`` pixels -> ``ModelView``.
        A ray is sampled every ``step`` (None: ``trunc / 2``) from ``near`` to ``far`` (None: ``TrackParams``' defaults):
        ``ceil((far - near) / step)`` samples, at most 4096.  ``colour`` False: no ``rgb``, and the colour planes are not read.
        ``out``: ``(xyz, normals, rgb, status, counts)`` contiguous device tensors of the result's shapes to write into (``rgb``
        None without colour).  ``clip`` False visits every sample instead of those inside the volume's box: the same bytes,
        more time (a measurement).  The volume is only read; no host read."""
        import torch
        p = self.params
        width, height = int(width), int(height)
        k = depth_frame.Intrinsics.coerce(intrinsics)
        if k is None or not (np.isfinite(k.astuple()).all() and k.fx != 0.0 and k.fy != 0.0):
            raise ValueError("raycast: the intrinsics must be finite with non-zero fx and fy")
        defaults = TrackParams()
        near = defaults.near if near is None else near
        far = defaults.far if far is None else far
        step = float(p.trunc) / 2.0 if step is None else step
        check_ray_range(near, far, step, "raycast")
        n_steps = ray_steps(near, far, step)
        if n_steps > MAX_RAY_STEPS:
            raise ValueError("raycast: %d samples per ray, more than %d; raise step or bring near and far together"
                             % (n_steps, MAX_RAY_STEPS))
        T = np.eye(4) if pose is None else matrix4(pose, "a pose must be a finite 4x4 camera-to-common transform", finite=True)
        with np.errstate(over="ignore"):
            rows = np.ascontiguousarray(T[:3, :].reshape(12).astype(np.float32))
            k4 = np.ascontiguousarray(np.array([1.0 / k.fx, 1.0 / k.fy, k.cx, k.cy], dtype=np.float64).astype(np.float32))
        if width < 1 or height < 1:
            raise ValueError("raycast: width and height must be at least 1")
        n = width * height
        dev = self.device
        shapes = (((n, 3), torch.float32), ((n, 3), torch.float32), ((n, 3), torch.float32), ((n,), torch.uint8),
                  ((4,), torch.int32))
        nx, ny, nz = p.dims
        with torch.cuda.device(dev), stream_scope(stream):
            if out is None:
                out = tuple(torch.empty(shape, dtype=dtype, device=dev) if colour or j != 2 else None
                            for j, (shape, dtype) in enumerate(shapes))
            if len(out) != 5 or (out[2] is None) != (not colour):
                raise ValueError("raycast: out must be (xyz, normals, rgb, status, counts), rgb None exactly without colour")
            for t, (shape, dtype) in zip(out, shapes):
                if t is not None and not (t.is_cuda and t.device == dev and tuple(t.shape) == shape and t.dtype == dtype
                                          and t.is_contiguous()):
                    raise ValueError("raycast: out must be contiguous device tensors (H W,3) x 3 float32, (H W) uint8, (4) int32")
            xyz, normals, rgb, status, counts = out
            _lib.call("regnet_tsdf_raycast_f32", self.data, self.data.data_ptr(), nx, ny, nz, self.origin.ctypes.data,
                      float(p.voxel), int(p.min_weight), k4.ctypes.data, rows.ctypes.data, float(near), float(step), n_steps,
                      width, height, 1 if clip else 0, xyz.data_ptr(), normals.data_ptr(),
                      None if rgb is None else rgb.data_ptr(), status.data_ptr(), counts.data_ptr(),
                      stream=None if stream is None else stream.cuda_stream)
            record_streams(stream, self.data, *out)
        return ModelView(xyz, normals, rgb, status, counts, width, height, k, T)

    def view_gain(self, poses, intrinsics, width, height, near=None, far=None, step=None, max_unknown=None, margin=0.0,
                  interest=None, status=True, clip=True, stream=None, out=None):
        """Per candidate camera pose (at most 32) the unobserved voxels its rays would reach -> ``view_plan.ViewGain``:
        ``view_plan.view_gain`` on this volume, which see.  The bit plane, 4 bytes per voxel, is allocated on the first call and
        kept on the volume, like the mesh's row plane."""
        from . import view_plan
        return view_plan.view_gain(self, poses, intrinsics, width, height, near, far, step, max_unknown, margin, interest,
                                   status, clip, stream, out)

    def distance_field(self, mode="solid", outside=None, margin=0.0, nearest=False, min_weight=None, stream=None, out=None,
                       signed=False, max_distance=None):
        """The exact Euclidean distance field of the volume as it stands -> ``DistanceField``: per voxel the squared distance, in
        voxels, to the nearest obstacle voxel (csrc/edt.hip).  ``mode``: ``"solid"`` -- the obstacles are the voxels seen solid,
        ``D < margin / trunc`` -- or ``"solid_or_unseen"``: those and the voxels observed fewer than ``min_weight`` (None: the
        volume's) times.  ``outside``: whether everything beyond the volume's six faces is an obstacle too; None: exactly with
        ``"solid_or_unseen"``.  ``nearest``: also keep, per voxel, which obstacle voxel that is.  ``out``: a ``DistanceField`` of
        this volume's dims whose buffers are written instead of new ones (4, with ``nearest`` 8 bytes per voxel).  Three
        launches, no host read.

        ``signed``: a SIGNED field (``regnet_tsdf_sdf``): an obstacle voxel holds minus its squared distance to the nearest
        non-obstacle voxel (and ``nearest`` the way out), every other voxel the distance above, now >= 1; 0 does not occur.  It
        takes a second transform over the complement (six launches) and a workspace as large as the field, kept on the result.
        ``max_distance`` (metres, > 0): a cap -- distances saturate at ``cap`` voxels, the smallest integer
        ``>= max_distance / voxel`` (1..1023), and no line search goes further than that: what bounds the cost wherever a
        plane holds no obstacle.  An ``out`` field must have been built ``signed`` to be reused for a signed one."""
        import torch
        p = self.params
        if mode not in FIELD_MODES:
            raise ValueError("distance_field: mode must be one of %s, not %r" % (", ".join(FIELD_MODES), mode))
        outside = (mode == "solid_or_unseen") if outside is None else bool(outside)
        min_weight = int(p.min_weight if min_weight is None else min_weight)
        signed = bool(signed)
        cap = field_cap(max_distance, p.voxel)
        nx, ny, nz = p.dims
        n = nx * ny * nz
        dev = self.device
        with torch.cuda.device(dev), stream_scope(stream):
            work = None
            if out is None:
                dist2 = torch.empty((n,), dtype=torch.int32, device=dev)
                near = torch.empty((n,), dtype=torch.int32, device=dev) if nearest else None
                if signed:
                    work = torch.empty((n * (2 if nearest else 1),), dtype=torch.int32, device=dev)
            else:
                if not isinstance(out, DistanceField) or out.dims != p.dims or out.dist2.device != dev:
                    raise ValueError("distance_field: out must be a DistanceField of this volume's dims on its device")
                if nearest and out.nearest is None:
                    raise ValueError("distance_field: out has no nearest plane")
                dist2, near = out.dist2, (out.nearest if nearest else None)
                if signed:
                    work = out.work
                    if work is None or work.numel() < n * (2 if nearest else 1):
                        raise ValueError("distance_field: out holds no workspace for a signed field%s; build it with signed=True"
                                         % (" with nearest" if nearest else ""))
            if signed or cap:
                _lib.call("regnet_tsdf_sdf", self.data, self.data.data_ptr(), nx, ny, nz, float(p.trunc), min_weight,
                          float(margin), FIELD_MODES.index(mode), int(outside), int(signed), cap, dist2.data_ptr(),
                          None if near is None else near.data_ptr(), None if work is None else work.data_ptr(),
                          stream=None if stream is None else stream.cuda_stream)
            else:
                _lib.call("regnet_tsdf_edt", self.data, self.data.data_ptr(), nx, ny, nz, float(p.trunc), min_weight,
                          float(margin), FIELD_MODES.index(mode), int(outside), dist2.data_ptr(),
                          None if near is None else near.data_ptr(), stream=None if stream is None else stream.cuda_stream)
            record_streams(stream, self.data, dist2, near, work)
        if out is not None:
            out.mode, out.outside, out.origin, out.voxel = mode, outside, self.origin, float(p.voxel)
            out.has_nearest = nearest
            out.signed, out.cap = signed, cap
            return out
        return DistanceField(dist2, near, p.dims, self.origin, float(p.voxel), mode, outside, signed=signed, cap=cap, work=work)


FIELD_MODES = ("solid", "solid_or_unseen")      # regnet_tsdf_edt's mode 0 and 1
EDT_NONE = 1 << 30                  # REGNET_EDT_NONE: the squared distance where there is no obstacle at all
MAX_FIELD_DIM = 1024                # regnet_tsdf_edt's documented limit on every dim
MAX_FIELD_CAP = 1023                # regnet_tsdf_sdf's largest cap, in voxels


def field_cap(max_distance, voxel):
    """``max_distance`` in metres -> the cap of ``regnet_tsdf_sdf`` in voxels: 0 for None, else the smallest integer
    ``>= max_distance / voxel`` (float64), which must lie in 1..1023."""
    if max_distance is None:
        return 0
    d = float(max_distance)
    if not (d > 0.0 and np.isfinite(d)):
        raise ValueError("distance_field: max_distance must be positive and finite, not %r" % (max_distance,))
    cap = int(np.ceil(d / float(voxel)))
    if not 1 <= cap <= MAX_FIELD_CAP:
        raise ValueError("distance_field: max_distance = %g m is %d voxels; the cap must lie in 1..%d" % (d, cap, MAX_FIELD_CAP))
    return cap


class DistanceField:
    """``Volume.distance_field``'s result, on the device.  ``dist2`` (N) int32: per voxel ``(iz ny + iy) nx + ix`` the squared
    distance in voxels (between voxel centres) to the nearest obstacle voxel, 0 on an obstacle, ``EDT_NONE`` = 2^30 when there is
    none; ``nearest`` (N) int32 or None: that obstacle's linear index -- of several at the same distance the smallest --, -1
    where there is none or the outside of the volume is strictly nearer.  ``dims``, ``origin`` (3 float32, host) and ``voxel`` are
    the volume's; ``mode`` and ``outside`` say what counted as an obstacle.  Unsigned by default: 0 everywhere inside an obstacle.

    ``signed``: ``dist2`` holds signed words instead -- minus the squared distance to the nearest NON-obstacle voxel on an obstacle
    voxel (``nearest``: that voxel, the way out), never 0, ``-EDT_NONE`` when no voxel is free.  ``cap``: 0, or the voxels at which
    the distances saturate (``cap * cap`` in ``dist2``, ``nearest`` -1 strictly beyond).  ``work``: the device workspace of the
    signed transform, kept for ``out=`` reuse (None for an unsigned field)."""

    def __init__(self, dist2, nearest, dims, origin, voxel, mode, outside, signed=False, cap=0, work=None):
        self.dist2, self.nearest, self.dims, self.origin, self.voxel = dist2, nearest, tuple(dims), origin, float(voxel)
        self.mode, self.outside = mode, bool(outside)
        self.signed, self.cap, self.work = bool(signed), int(cap), work
        self.has_nearest = nearest is not None      # (a reused field may hold a nearest plane its last call did not write)

    def bytes(self):
        """Bytes of the field on the device: 4 per voxel, 8 with ``nearest``, and the signed transform's workspace it keeps."""
        planes = int(self.dist2.numel()) * 4 * (1 if self.nearest is None else 2)
        return planes + (0 if self.work is None else int(self.work.numel()) * 4)

    def query(self, points, to_volume=None, nearest=False, stream=None, interpolate=False, gradient=False,
              gradient_frame="volume"):
        """``points`` (M,3) float32 on the field's device, any strides; ``to_volume``: the 4x4 that takes them into the volume's
        frame (None: identity; its rows 0..2 are rounded to float32 once).  -> ``distance`` (M) float32, metres to the nearest
        obstacle voxel's centre from the centre of the voxel the point lies in: ``+inf`` when there is no obstacle, NaN for a point
        outside the volume or not finite.  With ``nearest`` -> ``(distance, nearest_xyz)``, (M,3) float32: that obstacle voxel's
        centre in the volume's frame, NaN where there is none.  One launch, no host read.

        A SIGNED field answers through ``regnet_edt_query_signed_f32``: ``distance`` is the signed distance in metres to the
        boundary FACE between obstacle and free voxels (``(sqrt|s| - 0.5) voxel`` with the sign of the word), negative inside an
        obstacle.  ``interpolate``: trilinear between the eight voxel centres around the point instead of the nearest voxel's
        value (clamped in the outer half-voxel rim); an uncapped field has infinite words wherever a side is empty, and an
        interpolant that meets one is infinite or NaN, so build the field with ``max_distance`` for interpolated use.
        ``gradient`` (needs ``interpolate``): also return the (M,3) analytic derivative of the interpolant, dimensionless, of
        length 1 across a flat wall, pointing out of the obstacle; ``gradient_frame="volume"`` (bit-pinned) or ``"points"``:
        rotated into the points' frame by the transpose of ``to_volume``'s 3x3 with a torch product, which is NOT bit-pinned.
        The result is ``distance``, then ``gradient``, then ``nearest_xyz``, as many as were asked for."""
        import torch
        if gradient_frame not in ("volume", "points"):
            raise ValueError("query: gradient_frame must be \"volume\" or \"points\", not %r" % (gradient_frame,))
        if (interpolate or gradient) and not self.signed:
            raise ValueError("query: interpolate and gradient read a signed field; build it with signed=True")
        if gradient and not interpolate:
            raise ValueError("query: the gradient is the interpolant's; give interpolate=True with it")
        points = require_cuda("points", points, torch.float32, 3, error=TypeError)
        dev = self.dist2.device
        if points.device != dev:
            raise RuntimeError("query: the points are on %s, the field on %s" % (points.device, dev))
        if nearest and not self.has_nearest:
            raise ValueError("query: the field was built without nearest=True")
        T = np.eye(4) if to_volume is None else matrix4(to_volume, "to_volume must be a finite 4x4 transform", finite=True)
        with np.errstate(over="ignore"):
            rows = np.ascontiguousarray(T[:3, :].reshape(12).astype(np.float32))
        m = int(points.shape[0])
        nx, ny, nz = self.dims
        with torch.cuda.device(dev), stream_scope(stream):
            distance = torch.empty((m,), dtype=torch.float32, device=dev)
            xyz = torch.empty((m, 3), dtype=torch.float32, device=dev) if nearest else None
            grad = torch.empty((m, 3), dtype=torch.float32, device=dev) if gradient else None
            if self.signed:
                _lib.call("regnet_edt_query_signed_f32", self.dist2, self.dist2.data_ptr(),
                          self.nearest.data_ptr() if self.has_nearest else None, nx, ny, nz, self.origin.ctypes.data, self.voxel,
                          points.data_ptr(), points.stride(0), points.stride(1), m, rows.ctypes.data, int(bool(interpolate)),
                          distance.data_ptr(), None if grad is None else grad.data_ptr(),
                          None if xyz is None else xyz.data_ptr(), stream=None if stream is None else stream.cuda_stream)
                if grad is not None and gradient_frame == "points":
                    grad = grad @ torch.from_numpy(rows.reshape(3, 4)[:, :3].copy()).to(dev)   # row g R = (R^T g)^T
            else:
                _lib.call("regnet_edt_query_f32", self.dist2, self.dist2.data_ptr(),
                          self.nearest.data_ptr() if self.has_nearest else None, nx, ny, nz, self.origin.ctypes.data, self.voxel,
                          points.data_ptr(), points.stride(0), points.stride(1), m, rows.ctypes.data, distance.data_ptr(),
                          None if xyz is None else xyz.data_ptr(), stream=None if stream is None else stream.cuda_stream)
            record_streams(stream, points, self.dist2, self.nearest, distance, xyz, grad)
        result = (distance,) + ((grad,) if gradient else ()) + ((xyz,) if nearest else ())
        return result if len(result) > 1 else distance

    def metres(self, dist2=None, stream=None):
        """The whole field as (N) float32 metres, by the query's two operations -- ``sqrtf((float)dist2) * float32(voxel)``,
        ``+inf`` for ``EDT_NONE`` --: a dense grid to hand to a planner; ``view(nz, ny, nx)`` is its lattice.  ``dist2``: any
        contiguous int32 device tensor of squared distances to convert instead (a grasp's margins).  A signed field converts
        signed words: ``(sqrt|s| - 0.5) voxel`` with the sign of ``s``, the distance to the boundary face, ``-inf`` / ``+inf`` for
        ``-EDT_NONE`` / ``EDT_NONE``."""
        import torch
        source = self.dist2 if dist2 is None else dist2
        if not (source.is_cuda and source.dtype == torch.int32 and source.is_contiguous()):
            raise TypeError("metres: dist2 must be a contiguous int32 device tensor")
        with torch.cuda.device(source.device), stream_scope(stream):
            out = torch.empty(source.shape, dtype=torch.float32, device=source.device)
            _lib.call("regnet_edt_metres_signed_f32" if self.signed else "regnet_edt_metres_f32", source, source.data_ptr(),
                      int(source.numel()), self.voxel, out.data_ptr(),
                      stream=None if stream is None else stream.cuda_stream)
            record_streams(stream, source, out)
        return out


class Tracked:
    """``Tracker.track``'s result.  ``pose``: the tracker's pose after the frame, (4,4) float64 camera-to-common; ``status``:
    ``FIRST`` (the first frame, integrated at the starting pose), ``TRACKED`` (registered and integrated) or ``LOST`` (nothing
    integrated, the pose kept); ``report``: ``registration.decode_state``'s dict of the registration, whose ``pose`` takes the
    frame into the model view's camera (None for FIRST); ``counts``: integrate's (4) int32 on the device (None when LOST);
    ``model``: the ``ModelView`` the frame was registered against (None for FIRST), ``hits`` the pixels in which it hit;
    ``levels``: on the coarse-to-fine path a (levels, 2) int32 array, row ``l`` the ``(iteration, status)`` the registration
    stood at when level ``l`` had run -- row 0 is the end --, else None."""

    def __init__(self, pose, status, report, counts, model, hits=None, levels=None):
        self.pose, self.status, self.report, self.counts, self.model, self.hits = pose, status, report, counts, model, hits
        self.levels = levels


class Tracker:
    """One moving depth camera against one volume.  ``Tracker(tsdf_params, track_params, device, volume)`` holds a ``Volume``
    (``volume``: one to use, its parameters then hold; it is reset) that is NOT reset between frames, ``pose`` (4,4) float64,
    the camera-to-common pose of the last frame that was not lost, and ``frames``, the frames integrated.  ``depth_params`` go
    to ``depth_frame.to_cloud``."""

    def __init__(self, tsdf_params=None, track_params=None, device="cuda:0", volume=None, depth_params=None):
        self.params = TrackParams.coerce(track_params)
        self.volume = Volume(tsdf_params, device) if volume is None else volume
        self.device = self.volume.device
        self.depth_params = depth_params
        self.reset()

    def reset(self, pose=None, stream=None):
        """An empty volume, no frames, and ``pose`` (None: identity) as the pose the first frame is integrated at."""
        self.pose = np.eye(4) if pose is None else matrix4(pose, "a pose must be a finite 4x4 camera-to-common transform",
                                                           finite=True).copy()
        self.frames = 0
        self.volume.reset(stream=stream)

    def _cloud(self, frame, stream):
        import torch
        if isinstance(frame, depth_frame.DepthFrame):
            xyz, rgb = depth_frame.to_cloud(frame, self.depth_params, device=self.device, stream=stream)
            return xyz, rgb, int(frame.depth.shape[1]), int(frame.depth.shape[0]), frame.intrinsics
        if not isinstance(frame, (tuple, list)) or len(frame) != 5:
            raise TypeError("track takes a DepthFrame or (xyz, rgb, width, height, Intrinsics)")
        xyz, rgb, width, height, k = frame
        xyz = require_cuda("xyz", xyz, torch.float32, 3, error=TypeError).contiguous()
        if int(xyz.shape[0]) != int(width) * int(height):
            raise ValueError("track: xyz must be the organised cloud of its %d x %d frame" % (int(width), int(height)))
        return xyz, rgb, int(width), int(height), depth_frame.Intrinsics.coerce(k)

    def track(self, frame, guess=None, stream=None):
        """One frame (a ``depth_frame.DepthFrame``, or ``(xyz, rgb, width, height, Intrinsics)`` already on the device as
        ``Volume.integrate`` takes it) -> ``Tracked``.  The first frame is integrated at ``pose``.  A later one: the model view
        from ``guess`` (a camera-to-common 4x4; None: the last pose) with the frame's own intrinsics and size, the frame's cloud
        registered onto it from the identity, ONE blocking read (the registration's 1152-byte state and the view's 16-byte
        histogram, as one tensor), ``pose = pose_model @ T``, and the frame integrated there.  When the registration ends
        TOO_FEW or DEGENERATE, moved further than ``max_translation`` / ``max_rotation``, or the view hit in fewer than
        ``min_hit_share`` of its pixels, the frame is LOST: nothing is integrated and the pose is kept."""
        import torch
        from . import registration
        t = self.params
        xyz, rgb, width, height, k = self._cloud(frame, stream)
        view = (xyz, rgb, width, height, k)
        if self.frames == 0:
            counts = self.volume.integrate(view, self.pose, stream=stream)
            self.frames = 1
            return Tracked(self.pose.copy(), FIRST, None, counts, None)
        at = self.pose if guess is None else matrix4(guess, "a guess must be a finite 4x4 camera-to-common transform", finite=True)
        if t.pyramid():
            return self._track_pyramid(view, at, stream)
        model = self.volume.raycast(at, k, width, height, t.near, t.far, t.step, colour=False, stream=stream)
        icp = t.icp_params()
        n = int(xyz.shape[0])
        reg = registration.icp(xyz, model.target(icp, max_source=n, stream=stream), None, icp, stream=stream,
                               source_shape=(width, height))
        with torch.cuda.device(self.device), stream_scope(stream):
            both = torch.cat([reg.state, model.counts.view(torch.uint8)])
            record_streams(stream, both)
        raw = both.cpu().numpy()                             # the one blocking read
        report = registration.decode_state(raw[:registration.STATE_BYTES])
        hist = raw[registration.STATE_BYTES:].view(np.int32)
        hits = int(hist[HIT]) + int(hist[HIT_NO_NORMAL])
        return self._judge(view, at, report, model, hits, stream)


    def _judge(self, view, at, report, model, hits, stream, levels=None):
        """The gates, and the integration of a frame that passed them."""
        from . import registration
        t = self.params
        moved, turned = relative_motion(report["pose"])
        lost = (report["status"] in (registration.TOO_FEW, registration.DEGENERATE) or hits < t.min_hit_share * view[2] * view[3]
                or moved > t.max_translation or turned > t.max_rotation)
        if lost:
            return Tracked(self.pose.copy(), LOST, report, None, model, hits, levels)
        self.pose = at @ report["pose"]
        counts = self.volume.integrate(view, self.pose, stream=stream)
        self.frames += 1
        return Tracked(self.pose.copy(), TRACKED, report, counts, model, hits, levels)

    def _track_pyramid(self, view, at, stream):
        """``track`` coarse to fine (``TrackParams.levels`` / ``smooth``): the z column of the frame's cloud is its depth image;
        smoothed if asked, halved ``levels - 1`` times with the cutoff 3 ``sigma_depth`` (``max_dist`` without smoothing), every
        level deprojected by ``to_cloud`` and the model raycast at the level's intrinsics and size; the steps of every level,
        coarsest first, go onto ONE state block with ``registration.continue_state`` between two levels.  The one blocking read
        holds the state, level 0's histogram and the hand-over marks; the gates are ``track``'s, ``min_hit_share`` judged on
        level 0's view, and what is integrated is the frame's own cloud."""
        import torch
        from . import registration
        t = self.params
        xyz, _, width, height, k = view
        budgets = t.budgets()
        cutoff = t.smooth.cutoff() if t.smooth is not None else float(t.max_dist)
        with torch.cuda.device(self.device), stream_scope(stream):
            depth = xyz[:, 2].reshape(height, width).contiguous()
            marks = torch.zeros((t.levels, 2), dtype=torch.int32, device=self.device)
            state = to_device(registration.initial_state(None, t.icp_params(t.levels - 1)), self.device)
            record_streams(stream, xyz, depth, marks, state)
        pyramid = depth_frame.pyramid(depth, k, t.levels, cutoff, t.smooth, stream=stream)
        model = None
        for level in range(t.levels - 1, -1, -1):
            depth_l, k_l, w_l, h_l = pyramid[level]
            cloud, _ = depth_frame.to_cloud(depth_frame.DepthFrame(depth=depth_l, intrinsics=k_l), None, device=self.device,
                                            stream=stream)
            model = self.volume.raycast(at, k_l, w_l, h_l, t.near, t.far, t.step, colour=False, stream=stream)
            icp = t.icp_params(level)
            registration.icp(cloud, model.target(icp, max_source=w_l * h_l, stream=stream), None, icp, stream=stream, state=state,
                             source_shape=(w_l, h_l))
            if level > 0:
                registration.continue_state(state, budgets[level - 1], marks[level], stream=stream)
        with torch.cuda.device(self.device), stream_scope(stream):
            all_of_it = torch.cat([state, model.counts.view(torch.uint8), marks.view(torch.uint8).reshape(-1)])
            record_streams(stream, all_of_it)
        raw = all_of_it.cpu().numpy()                        # the one blocking read
        n_state = registration.STATE_BYTES
        report = registration.decode_state(raw[:n_state])
        hist = raw[n_state:n_state + 16].view(np.int32)
        levels = raw[n_state + 16:].view(np.int32).reshape(t.levels, 2).copy()
        levels[0] = (report["iterations"], report["status"])
        hits = int(hist[HIT]) + int(hist[HIT_NO_NORMAL])
        return self._judge(view, at, report, model, hits, stream, levels)


def relative_motion(T):
    """A rigid 4x4 -> (the length of its translation, its rotation angle [rad])."""
    cos = min(1.0, max(-1.0, (float(np.trace(T[:3, :3])) - 1.0) / 2.0))
    return float(np.linalg.norm(T[:3, 3])), math.acos(cos)


def fuse_volume(multiview, depth_params=None, tsdf_params=None, device="cuda:0", stream=None, register=None, volume=None,
                mesh=False, mesh_cell=None):
    """``depth_frame.to_cloud`` for every frame of ``multiview`` (a ``fusion.MultiView``), then reset, ``integrate`` in view order
    and ``extract`` -> ``Surface``, which carries ``counts`` (views,4) int32 on the device and ``volume``.  No host read.  With
    ``register`` (a ``registration.IcpParams`` or a dict of its fields) the poses go through ``fusion.refine_poses`` first -- its
    reads are then made -- and the result carries them: ``Surface.poses`` (V,4,4) float64 and ``Surface.register``, the (V,5)
    report.  ``volume``: a ``Volume`` to reuse instead of allocating one (its parameters then hold, and it is reset).  ``mesh``: ->
    ``(Surface, Mesh)`` of ``extract_mesh``; with ``mesh_cell`` [m] the second is its ``SimplifiedMesh`` (the full mesh is its
    ``source``), the ``Surface`` still the full one."""
    import torch
    from . import fusion
    if not isinstance(multiview, fusion.MultiView):
        raise TypeError("fuse_volume takes a MultiView")
    if mesh_cell is not None and not mesh:
        raise ValueError("fuse_volume: mesh_cell simplifies the mesh; give mesh=True")
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
    meshed = volume.extract_mesh(stream=stream) if mesh else None
    surface = meshed.surface if mesh else volume.extract(stream=stream)
    if mesh_cell is not None:
        meshed = meshed.simplify(cell=mesh_cell, stream=stream)
    with stream_scope(stream):
        surface.counts = torch.stack(counts)
    surface.volume = volume
    if report is not None:
        surface.poses, surface.register = np.stack(poses), report
    return (surface, meshed) if mesh else surface
