"""numpy restatement of the frame's side of coarse-to-fine tracking (include/regnet_hip.h, DESIGN.md par. 5 "Smoothing and the
pyramid"), written from the contract text and not from csrc/depth.hip or csrc/icp.hip: the bilateral filter, the 2 x 2 halving,
the level intrinsics, the hand-over of the state block between two levels, and the tracking loop around them.  float32 arrays,
one operation per statement (numpy rounds each on its own; its division is correctly rounded); the window is a Python loop over
its offsets, b outer and a inner, over ALL pixels at once.  The renderer of the model, the registration step and the volume are
``tsdf_raycast_reference``'s and ``icp_projective_reference``'s, imported and not copied.
"""
import math

import numpy as np

from . import depth_reference as dref
from . import icp_projective_reference as pref
from . import tsdf_raycast_reference as ray
from .icp_reference import CONVERGED, DEGENERATE, MAX_ITER, RUNNING, TOO_FEW

f32 = np.float32
QNAN = ray.QNAN
RANGE_BINS = 256
MAX_ITERATIONS = 64
SMOOTH_DEFAULTS = dict(radius=3, sigma_space=2.0, sigma_depth=0.01)
LEVEL_ITERATIONS = (10, 5, 4, 4)
PYRAMID_DEFAULTS = dict(levels=1, level_iterations=None, level_dist_scale=2.0, smooth=None)


def has_depth(z):
    """Finite and > 0."""
    with np.errstate(invalid="ignore"):
        return np.isfinite(z) & (z > 0)


def shifted(a, dy, dx, fill):
    """b[v, u] = a[v + dy, u + dx], ``fill`` beyond the image (a shift beyond the image's size leaves nothing but ``fill``)."""
    H, W = a.shape
    out = np.full_like(a, fill)
    if abs(dy) < H and abs(dx) < W:
        out[max(0, -dy):H - max(0, dy), max(0, -dx):W - max(0, dx)] = a[max(0, dy):H - max(0, -dy), max(0, dx):W - max(0, -dx)]
    return out


def tables(radius=3, sigma_space=2.0, sigma_depth=0.01):
    """-> (S (2r+1, 2r+1) float32, G (256,) float32, rbin float32): every entry evaluated in float64 and rounded once."""
    r = int(radius)
    S = np.empty((2 * r + 1, 2 * r + 1), dtype=np.float32)
    for b in range(-r, r + 1):
        for a in range(-r, r + 1):
            S[b + r, a + r] = f32(math.exp(-0.5 * (a * a + b * b) / (float(sigma_space) * float(sigma_space))))
    G = np.array([math.exp(-0.5 * (3.0 * (i + 0.5) / RANGE_BINS) ** 2) for i in range(RANGE_BINS)], dtype=np.float64).astype(np.float32)
    return S, G, f32(RANGE_BINS / (3.0 * float(sigma_depth)))


def smooth(depth, radius=3, sigma_space=2.0, sigma_depth=0.01):
    """The bilateral filter -> (H, W) float32, the quiet NaN where the centre has no depth."""
    z = np.asarray(depth, dtype=np.float32)
    assert z.ndim == 2
    r = int(radius)
    S, G, rbin = tables(r, sigma_space, sigma_depth)
    valid = has_depth(z)
    sw = np.zeros(z.shape, dtype=np.float32)
    sd = np.zeros(z.shape, dtype=np.float32)
    for b in range(-r, r + 1):
        for a in range(-r, r + 1):
            zq = shifted(z, b, a, f32(0))
            ok = valid & shifted(valid, b, a, False)
            with np.errstate(all="ignore"):
                d = zq - z
                t = np.abs(d) * rbin
                ok &= t < f32(256.0)
                w = S[b + r, a + r] * G[np.where(ok, t, f32(0)).astype(np.int64)]
                wd = w * d
                sw = np.where(ok, sw + w, sw)
                sd = np.where(ok, sd + wd, sd)
            assert d.dtype == t.dtype == w.dtype == wd.dtype == sw.dtype == sd.dtype == np.float32
    with np.errstate(all="ignore"):
        q = sd / sw
        out = z + q
    assert out.dtype == np.float32
    return np.where(valid, out, QNAN)


def halve(depth, cutoff):
    """One level of the pyramid -> (H // 2, W // 2) float32."""
    z = np.asarray(depth, dtype=np.float32)
    H, W = z.shape
    Ho, Wo = H // 2, W // 2
    with np.errstate(over="ignore"):
        cut = f32(cutoff)
    block = [z[0:2 * Ho:2, 0:2 * Wo:2], z[0:2 * Ho:2, 1:2 * Wo:2], z[1:2 * Ho:2, 0:2 * Wo:2], z[1:2 * Ho:2, 1:2 * Wo:2]]
    ref = np.full((Ho, Wo), np.inf, dtype=np.float32)
    for m in block:
        ref = np.where(has_depth(m) & (m < ref), m, ref)
    total = np.zeros((Ho, Wo), dtype=np.float32)
    count = np.zeros((Ho, Wo), dtype=np.int32)
    for m in block:
        with np.errstate(all="ignore"):
            gap = m - ref
            member = has_depth(m) & (gap <= cut)
            total = np.where(member, total + m, total)
        count += member
    assert total.dtype == np.float32
    with np.errstate(all="ignore"):
        mean = total / count.astype(np.float32)
    assert mean.dtype == np.float32
    return np.where(count > 0, mean, QNAN)


def level_intrinsics(k):
    """(fx / 2, fy / 2, (cx - 0.5) / 2, (cy - 0.5) / 2), in float64."""
    fx, fy, cx, cy = (float(v) for v in k)
    return (fx / 2.0, fy / 2.0, (cx - 0.5) / 2.0, (cy - 0.5) / 2.0)


def pyramid(depth, intrinsics, levels, cutoff, smooth_params=None):
    """-> [(depth_l, intrinsics_l, W_l, H_l)], finest first; ``smooth_params``: ``smooth``'s keywords, or None."""
    z = np.asarray(depth, dtype=np.float32)
    if smooth_params is not None:
        z = smooth(z, **dict(SMOOTH_DEFAULTS, **smooth_params))
    k = tuple(float(v) for v in intrinsics)
    out = [(z, k, z.shape[1], z.shape[0])]
    for _ in range(int(levels) - 1):
        z, k = halve(z, cutoff), level_intrinsics(k)
        out.append((z, k, z.shape[1], z.shape[0]))
    return out


def level_cloud(depth, intrinsics):
    """``to_cloud`` of a float32 depth image with default parameters -> (H W, 3) float32, quiet NaN rows without depth."""
    z = np.asarray(depth, dtype=np.float32)
    xyz = dref.deproject(z, intrinsics).reshape(-1, 3)
    return np.where(has_depth(z).reshape(-1, 1), xyz, QNAN)


def continue_state(iteration, status, max_iter, budget):
    """The hand-over -> (mark, status, max_iter): ``mark`` = (iteration, status) as found; CONVERGED and MAX_ITER run on with
    ``min(64, iteration + budget)`` as the new limit, every other status stays as it is."""
    assert 1 <= budget <= MAX_ITERATIONS
    mark = (int(iteration), int(status))
    if status in (CONVERGED, MAX_ITER):
        return mark, RUNNING, min(MAX_ITERATIONS, int(iteration) + int(budget))
    return mark, status, max_iter


def budgets(levels, level_iterations, iterations):
    if level_iterations is not None:
        return tuple(int(b) for b in level_iterations)
    return (int(iterations),) if levels == 1 else LEVEL_ITERATIONS[:levels]


def register_pyramid(vol, xyz, width, height, intrinsics, at, t, near_step_n, source_normals_of=None):
    """The registration of one frame, coarsest level first, on one state -> (report, model of level 0, marks (levels, 2))."""
    near, step, n_steps = near_step_n
    levels = int(t["levels"])
    b = budgets(levels, t["level_iterations"], t["iterations"])
    sm = t["smooth"]
    cutoff = 3.0 * float(dict(SMOOTH_DEFAULTS, **sm)["sigma_depth"]) if sm is not None else float(t["max_dist"])
    depth = np.asarray(xyz, dtype=np.float32).reshape(height, width, 3)[:, :, 2]
    pyr = pyramid(depth, intrinsics, levels, cutoff, sm)
    pose, status, it, max_iter = np.eye(4), RUNNING, 0, b[levels - 1]
    history = []
    marks = np.zeros((levels, 2), dtype=np.int32)
    model = None
    for level in range(levels - 1, -1, -1):
        z_l, k_l, w_l, h_l = pyr[level]
        cloud = level_cloud(z_l, k_l)
        model = ray.raycast(vol, at, k_l, w_l, h_l, near, step, n_steps, colour=False)
        params = {"max_dist": float(t["max_dist"]) * float(t["level_dist_scale"]) ** level, "stride": t["stride"],
                  "window": t["window"], "min_pairs": t["min_pairs"], "rot_eps": t["rot_eps"], "trans_eps": t["trans_eps"],
                  "min_cos": t["min_cos"], "iterations": max_iter}
        normals = None if t["min_cos"] is None else source_normals_of(cloud, w_l, h_l)
        for _ in range(b[level]):                              # the steps enqueued: one that finds the block ended does nothing
            if status != RUNNING:
                break
            pose, status, pairs, rms, _, _ = pref.step_projective(cloud, model["xyz"], model["normals"], w_l, h_l, k_l, pose, params,
                                                                  it, normals)
            history.append((float(pairs), rms))
            it += 1
        if level > 0:
            marks[level], status, max_iter = continue_state(it, status, max_iter, b[level - 1])
    marks[0] = (it, status)
    history = np.array(history, dtype=np.float64).reshape(-1, 2)
    ran = len(history) > 0
    report = {"pose": pose, "status": status, "iterations": it, "history": history, "pairs": int(history[-1, 0]) if ran else 0,
              "rms_first": float(history[0, 1]) if ran else 0.0, "rms_last": float(history[-1, 1]) if ran else 0.0}
    return report, model, marks


def track_pyramid(frames, width, height, intrinsics, volume_params, track_params=None, first_pose=None, guesses=None,
                  source_normals_of=None):
    """``tsdf_raycast_reference.track`` with the coarse-to-fine registration -> (Volume, [dict(pose, status, report, counts, model,
    levels)]).  ``track_params``: ``TRACK_DEFAULTS``' keys and ``PYRAMID_DEFAULTS``' (``smooth``: a dict of ``smooth``'s keywords or
    None); ``source_normals_of(cloud, W, H)``: the frame's normals per level when ``min_cos`` is set.  What is integrated is the
    frame's own cloud."""
    t = dict(ray.TRACK_DEFAULTS, **PYRAMID_DEFAULTS)
    t.update(track_params or {})
    vol = ray.Volume(**volume_params)
    step = float(vol.p["trunc"]) / 2.0 if t["step"] is None else float(t["step"])
    n = ray.steps(t["near"], t["far"], step)
    pose = np.eye(4) if first_pose is None else np.array(first_pose, dtype=np.float64)
    out = []
    for j, (xyz, rgb) in enumerate(frames):
        if j == 0:
            counts = vol.integrate(xyz, rgb, width, height, intrinsics, pose)
            out.append({"pose": pose.copy(), "status": ray.FIRST, "report": None, "counts": counts, "model": None, "levels": None})
            continue
        at = pose if guesses is None or guesses[j] is None else np.asarray(guesses[j], dtype=np.float64)
        reg, model, marks = register_pyramid(vol, xyz, width, height, intrinsics, at, t, (t["near"], step, n), source_normals_of)
        hits = int(model["counts"][ray.HIT]) + int(model["counts"][ray.HIT_NO_NORMAL])
        moved, turned = ray.relative_motion(reg["pose"])
        lost = (reg["status"] in (TOO_FEW, DEGENERATE) or hits < t["min_hit_share"] * width * height
                or moved > t["max_translation"] or turned > t["max_rotation"])
        if lost:
            out.append({"pose": pose.copy(), "status": ray.LOST, "report": reg, "counts": None, "model": model, "levels": marks})
            continue
        pose = at @ reg["pose"]
        counts = vol.integrate(xyz, rgb, width, height, intrinsics, pose)
        out.append({"pose": pose.copy(), "status": ray.TRACKED, "report": reg, "counts": counts, "model": model, "levels": marks})
    return vol, out
