"""The table plane of a camera frame, found on the device (csrc/plane.hip), and the table frame built on it: the calibration
``ingest.table_frame_transform()`` hard-codes for one camera.

``estimate_plane`` runs a seeded RANSAC over the frame (``hypotheses`` planes through three drawn points against every point,
inclusive threshold, optional gates on the plane's distance from the camera and on its tilt), then refits the winner's
inliers from ten float64 moments (summed once more in a fixed order, so the same cloud gives the same plane bit for bit) -- the only host read of the whole estimate, together with the winner's index and count
(96 bytes).  Everything that decides is canonical fp32 arithmetic (DESIGN.md par. 5, include/regnet_hip.h):
``tests/plane_reference.py`` restates it in numpy and the two agree exactly.  The draws come from a counter-based generator
of their own: numpy's global stream is not touched.  ``table_frame`` turns a plane into the 4x4 of
``table_frame_transform()``'s convention and ``calibrate`` does both.  GPU only: there is no CPU path.
"""
import math
from collections import namedtuple

import numpy as np

from . import _lib
from ._frame_util import MAX_FRAME_POINTS, require_cuda, to_device      # (MAX_*: regnet_plane_estimate_*'s documented limits)

_L = _lib.lib

MAX_HYPOTHESES = 4096
DEFAULT_THRESHOLD = 0.005
DEFAULT_HYPOTHESES = 1024
ALL_STAGES = 15

Plane = namedtuple("Plane", "normal offset inliers rms hypothesis")
Plane.__doc__ = """``normal`` (3,) float64, unit, pointing to the camera's side; ``offset`` = normal . x for the plane's points (so
the camera origin is at distance ``-offset`` above it); ``inliers``: the winner's count; ``rms`` of the inliers' distances to the
refitted plane [m]; ``hypothesis``: the winner's index."""
PlaneDetails = namedtuple("PlaneDetails", "counts hypotheses inlier_mask moments")


def workspace_bytes(M, hypotheses=DEFAULT_HYPOTHESES):
    """Bytes of scratch ``regnet_plane_estimate_*`` needs: 32 * hypotheses (-1 for unsupported sizes)."""
    return int(_L.regnet_plane_workspace_bytes(int(M), int(hypotheses)))


def cos2_tilt(max_tilt_deg):
    """cos^2 of the largest tilt, evaluated in float64 and rounded once to float32 (as a Python float)."""
    c = math.cos(math.radians(float(max_tilt_deg)))
    return float(np.float32(c * c))


def estimate_device(xyz, threshold=DEFAULT_THRESHOLD, hypotheses=DEFAULT_HYPOTHESES, seed=0, range=(0.0, math.inf),
                    up_hint=None, max_tilt_deg=None, stages=ALL_STAGES, out=None):
    """The kernels on their own: ``xyz`` (M,3) float32 / float64 GPU tensor -> ``(result, PlaneDetails, workspace)``, all on the device,
    on the current stream, no host read.  ``result`` is 96 bytes (uint8): the ten float64 moments, then int32 winner and
    count.  ``out``: a previous call's return value, to run without an allocation; ``stages``: see the header (measurements)."""
    import torch
    xyz = require_cuda("xyz", xyz, (torch.float32, torch.float64), 3).contiguous()
    M, H, dev = int(xyz.shape[0]), int(hypotheses), xyz.device
    if M > MAX_FRAME_POINTS:
        raise ValueError("frames of more than 2^21 points are not supported")
    if H <= 0 or H % 64 != 0 or H > MAX_HYPOTHESES:
        raise ValueError("hypotheses must be a multiple of 64, at most %d" % MAX_HYPOTHESES)
    seed = int(seed)
    if not 0 <= seed < 1 << 32:
        raise ValueError("seed must be in [0, 2^32)")
    lo, hi = (float(v) for v in range)
    if not (0.0 <= lo <= hi):
        raise ValueError("range must be 0 <= lo <= hi")
    if (up_hint is None) != (max_tilt_deg is None):
        raise ValueError("up_hint and max_tilt_deg go together")
    hint, c2 = None, 0.0
    if up_hint is not None:
        hint = np.ascontiguousarray(up_hint, dtype=np.float32)
        if hint.shape != (3,):
            raise ValueError("up_hint must be (3,)")
        c2 = cos2_tilt(max_tilt_deg)
    if out is None:
        result = torch.empty((96,), dtype=torch.uint8, device=dev)
        details = PlaneDetails(torch.empty((H,), dtype=torch.int32, device=dev),
                               torch.empty((H, 8), dtype=torch.float32, device=dev),
                               torch.empty((M,), dtype=torch.uint8, device=dev), result[:80].view(torch.float64))
        ws = torch.empty((workspace_bytes(M, H),), dtype=torch.uint8, device=dev)
    else:
        result, details, ws = out
    _lib.call("regnet_plane_estimate_f64" if xyz.dtype == torch.float64 else "regnet_plane_estimate_f32", xyz,
              xyz.data_ptr() if M else None, M, H, seed, float(threshold), lo, hi,
              hint.ctypes.data if hint is not None else None, c2, details.hypotheses.data_ptr(), details.counts.data_ptr(),
              details.inlier_mask.data_ptr() if M else None, result.data_ptr(), result.data_ptr() + 80, ws.data_ptr(),
              int(stages))
    return result, details, ws


def moments_fixed_order(xyz, inlier_mask, out=None):
    """regnet_plane_moments_det_*: the ten float64 moments of the rows of ``xyz`` (M,3) that ``inlier_mask`` (M) uint8 marks,
    summed in one fixed order, so that two estimates of one cloud agree bit for bit (the moments ``estimate_device`` leaves are
    added with float64 atomics in no fixed order).  -> (10,) float64 on the device (``out`` when given); no host read."""
    import torch
    M, dev = int(xyz.shape[0]), xyz.device
    if out is None:
        out = torch.empty((10,), dtype=torch.float64, device=dev)
    ws = torch.empty((int(_L.regnet_plane_moments_det_workspace_bytes(M)),), dtype=torch.uint8, device=dev)
    _lib.call("regnet_plane_moments_det_f64" if xyz.dtype == torch.float64 else "regnet_plane_moments_det_f32", xyz,
              xyz.data_ptr() if M else None, M, inlier_mask.data_ptr() if M else None, out.data_ptr(), ws.data_ptr())
    return out


def plane_from_moments(moments, hypothesis, inliers):
    """The refit on the host: ten float64 moments -> ``Plane``.  ``np.linalg.eigh`` of the covariance; the normal is the
    eigenvector of the smallest eigenvalue, signed so that the camera origin is on its positive side; rms = sqrt(eigenvalue)."""
    m = np.asarray(moments, dtype=np.float64)
    n = m[0]
    c = m[1:4] / n
    second = np.array([[m[4], m[5], m[6]], [m[5], m[7], m[8]], [m[6], m[8], m[9]]]) / n
    value, vector = np.linalg.eigh(second - np.outer(c, c))
    normal = vector[:, 0]
    offset = float(normal @ c)
    if offset > 0.0:                        # the origin's signed distance is -offset: keep it positive
        normal, offset = -normal, -offset
    return Plane(normal, offset, int(inliers), float(math.sqrt(max(value[0], 0.0))), int(hypothesis))


def estimate_plane(xyz, threshold=DEFAULT_THRESHOLD, hypotheses=DEFAULT_HYPOTHESES, seed=0, range=(0.0, math.inf),
                   up_hint=None, max_tilt_deg=None, return_details=False, device="cuda:0"):
    """The dominant plane of ``xyz`` (M,3), camera coordinates: a GPU tensor, or a host array / CPU tensor uploaded to
    ``device`` through ``host_io``; float32 or float64 (rounded once to float32); rows with a non-finite coordinate take no part.

    ``threshold`` [m]: a point within it (inclusive) is an inlier.  ``hypotheses``: a multiple of 64, at most 4096.  ``seed``
    in [0, 2^32) selects the draws.  ``range = (lo, hi)`` [m] gates the plane's distance from the camera origin: in a scene
    with a floor larger than the table the floor wins the plain count, so say roughly how far the table is.  ``up_hint`` (3)
    with ``max_tilt_deg``: only planes whose normal is within that angle of +-up_hint.  -> ``Plane``; with ``return_details``
    also ``PlaneDetails(counts (H) int32, hypotheses (H,8) float32, inlier_mask (M) uint8, moments (10) float64)`` on the
    device.  Raises ``ValueError`` when no plane is found (no eligible hypothesis with at least 3 inliers)."""
    import torch
    xyz = to_device(xyz, torch.device(device))
    result, details, _ = estimate_device(xyz, threshold, hypotheses, seed, range, up_hint, max_tilt_deg)
    moments_fixed_order(xyz, details.inlier_mask, out=details.moments)      # the refit's input, reproducible to the last bit
    host = result.cpu().numpy()                                    # the one blocking read: 96 bytes
    moments, (winner, count) = host[:80].view(np.float64), host[80:88].view(np.int32)
    if winner < 0:
        raise ValueError("estimate_plane: no plane found (no eligible hypothesis with at least 3 inliers)")
    plane = plane_from_moments(moments, winner, count)
    return (plane, details) if return_details else plane


def table_frame(plane, table_height=0.75):
    """``plane`` (a ``Plane``, or ``(normal, offset)``) -> the row-major 4x4 float64 camera -> table transform in the
    convention of ``ingest.table_frame_transform()``: z' is the plane normal, x' the camera's x axis projected into the plane
    and normalised (the camera's y axis when that projection is shorter than 1e-6), y' = z' x x', and the translation is
    (0, 0, table_height + the camera's distance to the plane): the plane lands at z = table_height and the camera origin
    above the frame's origin."""
    normal, offset = np.asarray(plane[0], dtype=np.float64), float(plane[1])
    length = np.linalg.norm(normal)
    z, offset = normal / length, offset / length
    x = np.array([1.0, 0.0, 0.0]) - z * z[0]
    if np.linalg.norm(x) < 1e-6:
        x = np.array([0.0, 1.0, 0.0]) - z * z[1]
    x = x / np.linalg.norm(x)
    y = np.cross(z, x)
    T = np.eye(4)
    T[0, :3], T[1, :3], T[2, :3] = x, y, z
    T[2, 3] = float(table_height) - offset
    return T


def calibrate(xyz, table_height=0.75, **estimate_kwargs):
    """``estimate_plane`` + ``table_frame`` -> ``(T, plane)``."""
    plane = estimate_plane(xyz, **estimate_kwargs)
    return table_frame(plane, table_height), plane
