"""What a depth camera delivers -- a 16-bit depth image, an 8-bit colour image, pinhole intrinsics -- turned into the organised
cloud ``ingest.crop_frame`` and ``table_plane.estimate_plane`` take, on the device (csrc/depth.hip): the step the reference did
with open3d before ``test.py`` ever saw a ``.pcd``.

``to_cloud`` uploads the images as they are (2 + 3 bytes per pixel, not 48), and one launch (three when the colour sensor has its
own pose) deprojects, removes flying pixels at depth discontinuities (``edge_threshold``, ``min_neighbours``) and colours the
points -- through a z-buffer of the colour camera when the sensors are not aligned, so that a foreground colour is not painted
on a background point the colour sensor cannot see.  Removed points are NaN rows, which every consumer treats as absent.
Everything that decides is canonical fp32 arithmetic (DESIGN.md par. 5, include/regnet_hip.h): ``tests/depth_reference.py``
restates it in numpy and the two agree bit for bit.  No host synchronisation, no host read.  GPU only: there is no CPU path.
"""
import math
from dataclasses import dataclass
from typing import Any, Optional, Tuple

import numpy as np

from . import _lib
from ._frame_util import MAX_FRAME_POINTS, ParamsBase, matrix4, record_streams, require_cuda, stream_scope, to_device, to_host

_L = _lib.lib

MAX_DEPTH_PIXELS = MAX_FRAME_POINTS         # regnet_depth_to_cloud_*'s documented limits
MAX_COLOR_PIXELS = 1 << 23
MODE_NONE, MODE_ALIGNED, MODE_REGISTERED = 0, 1, 2
STATUS = ("no depth", "out of range", "edge jump", "too few neighbours", "outside the colour image", "occluded", "kept")
KEPT = 6
NUM_PARAMS = 25


@dataclass(frozen=True)
class Intrinsics:
    """Pinhole intrinsics in pixels; no distortion model."""
    fx: float
    fy: float
    cx: float
    cy: float

    @classmethod
    def coerce(cls, value):
        if value is None or isinstance(value, cls):
            return value
        v = np.asarray(value, dtype=np.float64).reshape(-1)
        if v.shape != (4,):
            raise ValueError("intrinsics must be (fx, fy, cx, cy)")
        return cls(*(float(x) for x in v))

    def astuple(self):
        return (self.fx, self.fy, self.cx, self.cy)


@dataclass
class DepthFrame:
    """One frame of a depth camera.  ``depth`` (H, W): uint16 raw units (``z = depth * depth_scale`` metres, 0 = no depth) or
    float32 metres; ``color`` (H, W, 3) uint8 on the depth grid, or (Hc, Wc, 3) uint8 with ``color_intrinsics`` and the row-major
    4x4 ``depth_to_color`` transform of a colour sensor with its own pose.  Arrays may be numpy arrays or device tensors."""
    depth: Any
    intrinsics: Any
    color: Any = None
    color_intrinsics: Any = None
    depth_to_color: Any = None
    depth_scale: float = 0.001

    def __post_init__(self):
        self.intrinsics = Intrinsics.coerce(self.intrinsics)
        self.color_intrinsics = Intrinsics.coerce(self.color_intrinsics)
        if self.intrinsics is None:
            raise ValueError("DepthFrame: the depth intrinsics are required")

    def mode(self):
        """0 none / 1 aligned / 2 registered; a half-given colour camera is a ValueError."""
        has_k, has_t = self.color_intrinsics is not None, self.depth_to_color is not None
        if self.color is None:
            if has_k or has_t:
                raise ValueError("DepthFrame: color_intrinsics / depth_to_color without a colour image")
            return MODE_NONE
        if not has_k and not has_t:
            return MODE_ALIGNED
        if has_k and has_t:
            return MODE_REGISTERED
        raise ValueError("DepthFrame: a colour camera of its own needs both color_intrinsics and depth_to_color")


@dataclass(frozen=True)
class DepthParams(ParamsBase):
    """``depth_range = (lo, hi)`` [m], inclusive; ``edge_threshold`` t (None: off): a pixel is removed when an 8-neighbour's
    depth differs by more than t times the smaller of the two; ``min_neighbours`` k (0..8): a pixel with fewer valid 8-neighbours
    is removed; ``occlusion_margin`` [m] and ``splat`` (0..2, the z-buffer footprint's radius in colour pixels) govern the
    visibility test of a colour sensor with its own pose; ``keep_uncoloured``: points that sensor does not see keep their
    coordinates with rgb = 0 instead of being dropped."""
    WORD, NONE_IS_DEFAULT = "depth", True
    depth_range: Tuple[float, float] = (0.0, math.inf)
    edge_threshold: Optional[float] = None
    min_neighbours: int = 0
    occlusion_margin: float = 0.01
    splat: int = 1
    keep_uncoloured: bool = False

    def __post_init__(self):
        lo, hi = (float(v) for v in self.depth_range)
        if not (0.0 <= lo <= hi):
            raise ValueError("depth: depth_range must be 0 <= lo <= hi")
        object.__setattr__(self, "depth_range", (lo, hi))
        if self.edge_threshold is not None and not (float(self.edge_threshold) >= 0.0):
            raise ValueError("depth: edge_threshold must be None or >= 0")
        if int(self.min_neighbours) != self.min_neighbours or not 0 <= self.min_neighbours <= 8:
            raise ValueError("depth: min_neighbours must be in 0..8")
        if int(self.splat) != self.splat or not 0 <= self.splat <= 2:
            raise ValueError("depth: splat must be 0, 1 or 2")
        if not (float(self.occlusion_margin) >= 0.0):
            raise ValueError("depth: occlusion_margin must be >= 0")


def colour_lut():
    """The 256 entries float32(i / 255.0) the kernels hold in constant memory (the library's host copy)."""
    lut = np.empty((256,), dtype=np.float32)
    _L.regnet_depth_colour_lut(lut.ctypes.data)
    return lut


def workspace_bytes(width, height, color_width=0, color_height=0, mode=MODE_NONE):
    """Bytes of scratch ``regnet_depth_to_cloud_*`` needs: the z-buffer (4 Wc Hc rounded up to 16) in registered mode, 16
    otherwise; -1 for unsupported sizes."""
    return int(_L.regnet_depth_workspace_bytes(int(width), int(height), int(color_width), int(color_height), int(mode)))


def pack_params(frame, params, mode):
    """The 25 float32 constants of the C call: evaluated in float64, rounded once."""
    k = frame.intrinsics
    if not (k.fx != 0.0 and k.fy != 0.0):
        raise ValueError("depth: fx and fy must not be zero")
    p = np.zeros((NUM_PARAMS,), dtype=np.float64)
    p[0:5] = (1.0 / float(k.fx), 1.0 / float(k.fy), k.cx, k.cy, float(frame.depth_scale))
    p[5:7] = params.depth_range
    p[7] = 0.0 if params.edge_threshold is None else float(params.edge_threshold)
    p[8] = params.occlusion_margin
    if mode == MODE_REGISTERED:
        T = matrix4(frame.depth_to_color, "depth_to_color must be 4x4")
        p[9:13] = frame.color_intrinsics.astuple()
        p[13:22] = T[:3, :3].reshape(9)
        p[22:25] = T[:3, 3]
    with np.errstate(over="ignore"):
        return np.ascontiguousarray(p.astype(np.float32))


def _image(a, device, what, dtypes):
    """A host array or tensor -> a contiguous device tensor of one of ``dtypes`` (host arrays go up once, as they are)."""
    import torch
    if not isinstance(a, torch.Tensor) and np.asarray(a).dtype == np.float64 and torch.float32 in dtypes:
        a = np.asarray(a, dtype=np.float32)
    t = to_device(a, device)
    if t.dtype == torch.int16 and torch.uint16 in dtypes:
        t = t.view(torch.uint16)
    if t.dtype not in dtypes:
        raise TypeError("%s must be %s" % (what, " or ".join(str(d).replace("torch.", "") for d in dtypes)))
    return t


def to_cloud(frame, params=None, device="cuda:0", stream=None, return_status=False, out=None):
    """``frame`` (a ``DepthFrame``) -> ``(xyz, rgb)``: (H W, 3) float32 device tensors, row ``v W + u`` for pixel (u, v); a row
    that was removed holds NaN coordinates and rgb = 0.  With ``return_status`` also ``status`` (H W) uint8 (``STATUS``'s codes)
    and ``counts`` (8) int32, its histogram, both on the device.  ``params``: a ``DepthParams``, a dict of its fields or None.
    Host images go up once through ``host_io`` as uint16 / float32 and uint8; device tensors are used where they are (then the
    call is on their device).  ``stream``: a ``torch.cuda.Stream`` (default: the current one).  ``out``: a previous call's
    ``(xyz, rgb, status, counts, workspace)`` to run without an allocation.  No host synchronisation."""
    import torch
    if not isinstance(frame, DepthFrame):
        raise TypeError("to_cloud takes a DepthFrame")
    params = DepthParams.coerce(params)
    mode = frame.mode()
    dev = frame.depth.device if isinstance(frame.depth, torch.Tensor) and frame.depth.is_cuda else torch.device(device)
    if dev.type != "cuda":
        raise RuntimeError("to_cloud: the device must be a GPU (no CPU path)")
    scale = float(frame.depth_scale)
    if not (scale > 0.0 and math.isfinite(scale)):
        raise ValueError("depth_scale must be positive and finite")
    consts = pack_params(frame, params, mode)
    with stream_scope(stream):
        depth = _image(frame.depth, dev, "depth", (torch.uint16, torch.float32))
        if depth.dim() != 2 or depth.shape[0] < 1 or depth.shape[1] < 1:
            raise ValueError("depth must be (H, W) with at least one pixel")
        H, W = int(depth.shape[0]), int(depth.shape[1])
        if W * H > MAX_DEPTH_PIXELS:
            raise ValueError("depth images of more than 2^21 pixels are not supported")
        color, Wc, Hc = None, 0, 0
        if mode != MODE_NONE:
            color = _image(frame.color, dev, "color", (torch.uint8,))
            if color.dim() != 3 or color.shape[2] != 3 or color.shape[0] < 1 or color.shape[1] < 1:
                raise ValueError("color must be (H, W, 3) uint8")
            Hc, Wc = int(color.shape[0]), int(color.shape[1])
            if mode == MODE_ALIGNED and (Hc, Wc) != (H, W):
                raise ValueError("a colour image without intrinsics of its own must have the depth image's shape")
            if Wc * Hc > MAX_COLOR_PIXELS:
                raise ValueError("colour images of more than 2^23 pixels are not supported")
        if out is None:
            xyz = torch.empty((H * W, 3), dtype=torch.float32, device=dev)
            rgb = torch.empty((H * W, 3), dtype=torch.float32, device=dev)
            status = torch.empty((H * W,), dtype=torch.uint8, device=dev)
            counts = torch.empty((8,), dtype=torch.int32, device=dev)
            ws = torch.empty((workspace_bytes(W, H, Wc, Hc, mode),), dtype=torch.uint8, device=dev)
        else:
            xyz, rgb, status, counts, ws = out
        _lib.call("regnet_depth_to_cloud_u16" if depth.dtype == torch.uint16 else "regnet_depth_to_cloud_f32", depth,
                  depth.data_ptr(), W, H, consts.ctypes.data, color.data_ptr() if color is not None else None, Wc, Hc, mode,
                  0 if params.edge_threshold is None else 1, int(params.min_neighbours), int(params.splat),
                  1 if params.keep_uncoloured else 0, xyz.data_ptr(), rgb.data_ptr(), status.data_ptr(), counts.data_ptr(),
                  ws.data_ptr())
        record_streams(stream, depth, color)       # the inputs are read on `stream`: keep them alive for it
    return (xyz, rgb, status, counts) if return_status else (xyz, rgb)


def normals(xyz, width, height, step=2, max_jump=0.02, stream=None):
    """The normals of an organised cloud from its own pixel grid (regnet_depth_normals_f32): ``xyz`` (H W, 3) float32 on the
    device, row ``v W + u`` for pixel (u, v), as ``to_cloud`` gives it -> (H W, 3) float32 on the device.  A normal is the cross
    product of the differences ``step`` pixels along the image row and column, of length 1 and facing the camera at the origin;
    a neighbour whose depth differs from the centre's by more than ``max_jump`` [m] is left out (one-sided then), and a pixel
    without a normal -- removed itself, or without a neighbour along either axis -- holds three NaNs.  One launch, no host read."""
    import torch
    require_cuda("xyz", xyz, torch.float32, 3)
    width, height = int(width), int(height)
    if width < 1 or height < 1 or int(xyz.shape[0]) != width * height:
        raise ValueError("normals: xyz must have width * height rows")
    xyz = xyz.contiguous()
    with torch.cuda.device(xyz.device), stream_scope(stream):
        out = torch.empty((width * height, 3), dtype=torch.float32, device=xyz.device)
        _lib.call("regnet_depth_normals_f32", xyz, xyz.data_ptr(), width, height, int(step), float(max_jump), out.data_ptr(),
                  stream=None if stream is None else stream.cuda_stream)
        record_streams(stream, xyz)
    return out


MAX_SMOOTH_RADIUS = 4               # regnet_depth_bilateral_f32's documented limits
RANGE_BINS = 256


@dataclass(frozen=True)
class SmoothParams(ParamsBase):
    """The bilateral filter ``smooth`` applies to a depth image before it is tracked (``tsdf.TrackParams.smooth``; a dict with
    these keys works too).  ``radius`` (1..4): the window is (2 radius + 1)^2 pixels; ``sigma_space`` [pixels]: the Gaussian over
    the pixel distance; ``sigma_depth`` [m]: the Gaussian over the depth difference, cut to exactly zero beyond three of it, so
    nothing is averaged across a depth edge higher than that.

    Every default is a choice -- a 7 x 7 window, two pixels, a centimetre: the noise of a commodity depth camera at arm's
    length -- and not a measurement on real cameras."""
    WORD = "smooth"
    radius: int = 3
    sigma_space: float = 2.0
    sigma_depth: float = 0.01

    def __post_init__(self):
        if int(self.radius) != self.radius or not 1 <= self.radius <= MAX_SMOOTH_RADIUS:
            raise ValueError("smooth: radius must be in 1..%d" % MAX_SMOOTH_RADIUS)
        for name in ("sigma_space", "sigma_depth"):
            v = float(getattr(self, name))
            if not (v > 0.0 and math.isfinite(v)):
                raise ValueError("smooth: %s must be positive and finite" % name)
        with np.errstate(over="ignore", under="ignore"):
            rbin = np.float32(self.rbin())
        if not (rbin > 0.0 and np.isfinite(rbin)):
            raise ValueError("smooth: 256 / (3 sigma_depth) must be positive and finite in float32")

    def rbin(self):
        """Bins of the range table per metre, in float64: 256 / (3 sigma_depth)."""
        return RANGE_BINS / (3.0 * float(self.sigma_depth))

    def cutoff(self):
        """Three ``sigma_depth``: beyond it a neighbour has no weight, and the pyramid takes it as its cutoff."""
        return 3.0 * float(self.sigma_depth)


def smooth_tables(params=None):
    """The tables of regnet_depth_bilateral_f32 as ((2 radius + 1)^2 + 256,) float32 on the host, evaluated in float64 and rounded
    once per entry: ``S[b][a] = exp(-0.5 (a^2 + b^2) / sigma_space^2)`` row-major, then ``G[i] = exp(-0.5 (3 (i + 0.5) / 256)^2)``."""
    params = SmoothParams.coerce(params) or SmoothParams()
    r = int(params.radius)
    a = np.arange(-r, r + 1, dtype=np.float64)
    s = np.exp(-0.5 * (a[None, :] ** 2 + a[:, None] ** 2) / float(params.sigma_space) ** 2)
    g = np.exp(-0.5 * (3.0 * (np.arange(RANGE_BINS, dtype=np.float64) + 0.5) / RANGE_BINS) ** 2)
    return np.ascontiguousarray(np.concatenate([s.reshape(-1), g]).astype(np.float32))


def _depth_image(name, depth):
    """``depth`` must be an (H, W) float32 device tensor -> (contiguous tensor, W, H)."""
    import torch
    if not isinstance(depth, torch.Tensor) or not depth.is_cuda:
        raise RuntimeError("%s: depth must be a CUDA tensor (no CPU path)" % name)
    if depth.dtype != torch.float32 or depth.dim() != 2:
        raise TypeError("%s: depth must be (H, W) float32" % name)
    return depth.contiguous(), int(depth.shape[1]), int(depth.shape[0])


def _image_out(name, out, depth, height, width):
    import torch
    if out is None:
        return torch.empty((height, width), dtype=torch.float32, device=depth.device)
    if not (isinstance(out, torch.Tensor) and out.is_cuda and out.device == depth.device and out.dtype == torch.float32
            and tuple(out.shape) == (height, width) and out.is_contiguous()):
        raise ValueError("%s: out must be a contiguous (%d, %d) float32 tensor on the depth's device" % (name, height, width))
    if out.data_ptr() == depth.data_ptr():
        raise ValueError("%s: out must not be the input" % name)
    return out


def smooth(depth, params=None, stream=None, out=None, tables=None):
    """The bilateral filter of a depth image (regnet_depth_bilateral_f32): ``depth`` (H, W) float32 metres on the device -> (H, W)
    float32 on the device, NaN where the input has no depth (not finite, or <= 0): holes neither fill nor grow.  ``tables``: the
    device copy of ``smooth_tables(params)`` to reuse instead of uploading one.  One launch, no host read."""
    import torch
    params = SmoothParams.coerce(params) or SmoothParams()
    depth, W, H = _depth_image("smooth", depth)
    if W < 1 or H < 1 or W * H > MAX_DEPTH_PIXELS:
        raise ValueError("smooth: depth must have 1..2^21 pixels")
    with torch.cuda.device(depth.device), stream_scope(stream):
        if tables is None:
            tables = to_device(smooth_tables(params), depth.device)
        if not (tables.is_cuda and tables.device == depth.device and tables.dtype == torch.float32 and tables.is_contiguous()
                and tables.numel() == (2 * int(params.radius) + 1) ** 2 + RANGE_BINS):
            raise ValueError("smooth: tables must be smooth_tables(params) on the depth's device")
        out = _image_out("smooth", out, depth, H, W)
        _lib.call("regnet_depth_bilateral_f32", depth, depth.data_ptr(), W, H, int(params.radius), tables.data_ptr(),
                  float(params.rbin()), out.data_ptr(), stream=None if stream is None else stream.cuda_stream)
        record_streams(stream, depth, tables, out)
    return out


_smooth_image = smooth              # (``pyramid`` has a parameter of that name)


def halve(depth, cutoff, stream=None, out=None):
    """One level of the pyramid (regnet_depth_halve_f32): ``depth`` (H, W) float32 on the device -> (H // 2, W // 2) float32 on the
    device.  A coarse pixel is the mean of those valid pixels of its 2 x 2 block that lie within ``cutoff`` [m] (inclusive) behind
    the nearest of them, NaN when the block has none.  One launch, no host read."""
    import torch
    depth, W, H = _depth_image("halve", depth)
    if W < 2 or H < 2 or W * H > MAX_DEPTH_PIXELS:
        raise ValueError("halve: depth must be at least 2 x 2 and have at most 2^21 pixels")
    with np.errstate(over="ignore", under="ignore"):
        cut32 = np.float32(cutoff)
    if not (float(cutoff) > 0.0 and cut32 > 0.0 and np.isfinite(cut32)):
        raise ValueError("halve: cutoff must be positive and finite in float32")
    with torch.cuda.device(depth.device), stream_scope(stream):
        out = _image_out("halve", out, depth, H // 2, W // 2)
        _lib.call("regnet_depth_halve_f32", depth, depth.data_ptr(), W, H, float(cutoff), out.data_ptr(),
                  stream=None if stream is None else stream.cuda_stream)
        record_streams(stream, depth, out)
    return out


def level_intrinsics(k):
    """The intrinsics of the next coarser level, in float64: ``fx / 2, fy / 2, (cx - 0.5) / 2, (cy - 0.5) / 2``.  Pixel centres
    sit at integers, so coarse pixel u is the ray through fine coordinate 2u + 0.5."""
    k = Intrinsics.coerce(k)
    return Intrinsics(k.fx / 2.0, k.fy / 2.0, (k.cx - 0.5) / 2.0, (k.cy - 0.5) / 2.0)


def pyramid(depth, intrinsics, levels, cutoff, smooth=None, stream=None):
    """``depth`` (H, W) float32 on the device, smoothed first when ``smooth`` (a ``SmoothParams`` or a dict) is given, and its
    ``levels`` - 1 halvings -> a list of ``(depth_l, Intrinsics_l, W_l, H_l)``, finest first.  No host read."""
    levels = int(levels)
    if levels < 1:
        raise ValueError("pyramid: levels must be at least 1")
    k = Intrinsics.coerce(intrinsics)
    depth, W, H = _depth_image("pyramid", depth)
    if W >> (levels - 1) < 1 or H >> (levels - 1) < 1:
        raise ValueError("pyramid: a %d x %d image has no %d levels" % (W, H, levels))
    if smooth is not None:
        depth = _smooth_image(depth, smooth, stream=stream)
    out = [(depth, k, W, H)]
    for _ in range(levels - 1):
        depth, k, W, H = halve(depth, cutoff, stream=stream), level_intrinsics(k), W // 2, H // 2
        out.append((depth, k, W, H))
    return out


_NPZ_KEYS = ("depth", "intrinsics", "color", "color_intrinsics", "depth_to_color", "depth_scale")


def frame_items(frame, prefix=""):
    """The ``.npz`` entries of one ``DepthFrame``, their names behind ``prefix``: ``depth``, ``intrinsics`` (4), ``depth_scale``
    and, where given, ``color``, ``color_intrinsics`` (4), ``depth_to_color`` (4,4)."""
    items = {"depth": to_host(frame.depth), "intrinsics": np.array(frame.intrinsics.astuple(), dtype=np.float64),
             "depth_scale": np.float64(frame.depth_scale)}
    if frame.color is not None:
        items["color"] = to_host(frame.color)
    if frame.color_intrinsics is not None:
        items["color_intrinsics"] = np.array(frame.color_intrinsics.astuple(), dtype=np.float64)
    if frame.depth_to_color is not None:
        items["depth_to_color"] = to_host(frame.depth_to_color).astype(np.float64)
    return {prefix + key: value for key, value in items.items()}


def frame_from_items(data, prefix, path, required=("depth", "intrinsics")):
    """The ``DepthFrame`` of ``data``'s entries behind ``prefix`` (``path`` names the file in the error); a ``required`` entry
    that is missing is a ValueError."""
    for key in required:
        if prefix + key not in data.files:
            raise ValueError("%s: no %r entry" % (path, prefix + key))
    get = lambda key: data[prefix + key] if prefix + key in data.files else None      # noqa: E731
    scale = get("depth_scale")
    return DepthFrame(depth=get("depth"), intrinsics=get("intrinsics"), color=get("color"),
                      color_intrinsics=get("color_intrinsics"), depth_to_color=get("depth_to_color"),
                      depth_scale=0.001 if scale is None else float(scale))


def check_npz_entries(data, known, path):
    """Entries of ``data`` outside ``known`` are a ValueError (``path`` names the file)."""
    unknown = sorted(set(data.files) - set(known))
    if unknown:
        raise ValueError("%s: unknown entries %s" % (path, ", ".join(unknown)))


def save_npz(path, frame):
    """Write ``frame`` as a ``.npz``: ``frame_items``' entries."""
    with open(path, "wb") as f:
        np.savez(f, **frame_items(frame))


def load_npz(path):
    """Read a ``.npz`` written by ``save_npz`` (or by anything that uses its keys) -> ``DepthFrame``."""
    with np.load(path, allow_pickle=False) as data:
        check_npz_entries(data, _NPZ_KEYS, "depth frame %s" % path)
        return frame_from_items(data, "", "depth frame %s" % path)
