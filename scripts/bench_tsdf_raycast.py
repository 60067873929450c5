"""What the raycast of the TSDF volume and one tracked frame cost on the MI355X (tsdf.py, csrc/tsdf.hip) ->
profiles/tsdf_raycast.txt.

The two rendered 640 x 480 views of scripts/bench_tsdf.py in the default volume (320^3 voxels of 2 mm) moved onto the scene:
``Volume.raycast`` from the first view's pose with and without colour, with and without the clip against the box of voxel
centres; then one ``Tracker.track`` call of the second view after the first, and its parts on their own (``to_cloud``, the
raycast, the registration's enqueued steps, the blocking read, ``integrate``).  HIP-event times: warm-up first, then the median
of repeated runs with their min / max.  Beside the raycast times the samples the rays visit and the corner loads they make,
COUNTED by a march of the same rays in torch ops (``torch_march``: ``grid_sample`` over ``D`` and over the mask of observed
voxels, a Python loop over the samples) with the kernel's clip restated in float64 (``clip_range``): counts, not measured
traffic.  That march is also the comparison line: the same depth image by plumbing alone.  Last, one ``detect`` of a
``DepthFrame`` by a detector with ``track`` against one with ``volume`` (a one-view ``MultiView``), alternated, host clock.

    python scripts/bench_tsdf_raycast.py [--out profiles/tsdf_raycast.txt]
"""
import argparse
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_outliers import fmt, timed  # noqa: E402
from bench_tsdf import DEV, HEIGHT, ORIGIN, WIDTH, scene  # noqa: E402


def clip_range(pose, k, width, height, near, step, n_steps, origin, voxel, dims):
    """csrc/tsdf.hip ``rc_clip`` in numpy float64 -> (first, last) per pixel, last < first where the ray misses the box."""
    import numpy as np
    f = np.float32
    r = np.asarray(pose, dtype=np.float64)[:3, :].astype(f).astype(np.float64)
    k4 = np.array([1.0 / k.fx, 1.0 / k.fy, k.cx, k.cy]).astype(f)
    v, u = np.divmod(np.arange(width * height), width)
    dcx = (u.astype(f) - k4[2]).astype(np.float64) * float(k4[0])
    dcy = (v.astype(f) - k4[3]).astype(np.float64) * float(k4[1])
    near, step, vx = float(f(near)), float(f(step)), float(f(voxel))
    far = near + (n_steps - 1) * step
    slack = 2.0 ** -18
    za = np.full(dcx.shape, near - slack * (abs(near) + far))
    zb = np.full(dcx.shape, far + slack * (abs(near) + far))
    empty = np.zeros(dcx.shape, dtype=bool)
    with np.errstate(all="ignore"):
        for a in range(3):
            d = (r[a, 0] * dcx + r[a, 1] * dcy) + r[a, 2]
            o, extent = float(f(origin[a])), dims[a] * vx
            m = vx + slack * (abs(r[a, 3]) + (np.abs(r[a, 0] * dcx) + np.abs(r[a, 1] * dcy) + abs(r[a, 2])) * far + abs(o) + extent)
            lo, hi = o + 0.5 * vx - m, o + extent - 0.5 * vx + m
            z1, z2 = (lo - r[a, 3]) / d, (hi - r[a, 3]) / d
            flat = d == 0.0
            empty |= flat & ((r[a, 3] < lo) | (r[a, 3] > hi))
            za = np.where(flat, za, np.fmax(za, np.fmin(z1, z2)))
            zb = np.where(flat, zb, np.fmin(zb, np.fmax(z1, z2)))
        empty |= za > zb
        first = np.clip(np.floor((za - near) / step) - 1.0, 0.0, n_steps - 1.0)
        last = np.clip(np.ceil((zb - near) / step) + 1.0, 0.0, n_steps - 1.0)
    return np.where(empty, 1, first).astype(np.int64), np.where(empty, 0, last).astype(np.int64)


def torch_march(vol, pose, k, width, height, near, step, n_steps, first=None, last=None):
    """The raycast's march in torch ops: per sample one ``grid_sample`` of ``D`` and one of the observed-voxel mask (a sample
    is known where the mask interpolates to 1 within 1e-4), a Python loop over the samples -> (depth image (H W) with NaN where no hit,
    counts: samples visited by rays still marching, of those inside ``first..last``, inside the box of voxel centres, known)."""
    import torch
    p = vol.params
    nx, ny, nz = p.dims
    dev = vol.device
    D = vol.D.view(1, 1, nz, ny, nx)
    M = (vol.W >= p.min_weight).float().view(1, 1, nz, ny, nx)
    T = torch.tensor(pose, dtype=torch.float32, device=dev)
    v, u = torch.meshgrid(torch.arange(height, device=dev), torch.arange(width, device=dev), indexing="ij")
    ray = torch.stack([(u.reshape(-1) - k.cx) / k.fx, (v.reshape(-1) - k.cy) / k.fy, torch.ones(width * height, device=dev)], dim=1).float()
    ray = ray @ T[:3, :3].T
    origin = torch.tensor(p.origin, dtype=torch.float32, device=dev)
    top = torch.tensor([nx - 1, ny - 1, nz - 1], dtype=torch.float32, device=dev)
    n = width * height
    alive = torch.ones(n, dtype=torch.bool, device=dev)
    previous = torch.zeros(n, dtype=torch.bool, device=dev)
    v_prev, z_prev = torch.zeros(n, device=dev), torch.zeros(n, device=dev)
    depth = torch.full((n,), float("nan"), device=dev)
    counted = first is not None
    if counted:
        first, last = torch.from_numpy(first).to(dev), torch.from_numpy(last).to(dev)
    visited = clipped = inside_n = known_n = torch.zeros((), dtype=torch.int64, device=dev)
    for i in range(n_steps):
        z = near + i * step
        g = (ray * z + T[:3, 3] - origin) / p.voxel - 0.5
        grid = (2.0 * g / top - 1.0).view(1, 1, 1, n, 3)
        value = torch.nn.functional.grid_sample(D, grid, mode="bilinear", padding_mode="zeros", align_corners=True).view(n)
        mask = torch.nn.functional.grid_sample(M, grid, mode="bilinear", padding_mode="zeros", align_corners=True).view(n)
        inside = ((g >= 0) & (g < top)).all(dim=1)
        known = inside & (mask > 0.9999)      # (eight observed corners interpolate to 1 up to rounding)
        if counted:
            within = alive & (first <= i) & (last >= i)
            visited = visited + alive.sum()
            clipped = clipped + within.sum()
            inside_n = inside_n + (within & inside).sum()
            known_n = known_n + (within & known).sum()
        below = alive & known & (value <= 0)
        hit = below & previous
        depth = torch.where(hit, z_prev + v_prev / (v_prev - value) * step, depth)
        alive = alive & ~below
        previous = known & (value > 0)
        v_prev, z_prev = value, torch.full_like(z_prev, z)
    return depth, (visited, clipped, inside_n, known_n)


def detect_lines(mv):
    """One ``detect`` of the first view as a ``DepthFrame`` by a detector with ``track`` (its second call: a tracked frame)
    against one with ``volume`` given the same view as a one-view ``MultiView``, alternated, host clock."""
    import numpy as np
    import torch
    from regnet_for_3d_grasping_amd import detect, fusion, pipeline, tsdf
    score_net, region_net = pipeline.build_models(DEV)
    volume = tsdf.TsdfParams(origin=ORIGIN)
    common = dict(transform={"range": (0.5, 1.2)}, volume=volume)
    tracking = detect.GraspDetector(score_net, region_net, track={"near": 0.5, "far": 1.5}, **common)
    plain = detect.GraspDetector(score_net, region_net, **common)
    one = fusion.MultiView([mv.frames[0]], [None])
    times = {"track": [], "volume": []}
    status = None
    for j in range(8):
        for name, detector, frame in (("track", tracking, mv.frames[0]), ("volume", plain, one)):
            np.random.seed(7)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = detector.detect(frame)
            torch.cuda.synchronize()
            if j >= 2:
                times[name].append((time.perf_counter() - t0) * 1e3)
            if name == "track":
                status = int(out["track_status"])
    a, b = statistics.median(times["track"]), statistics.median(times["volume"])
    return ["detect of one 640 x 480 DepthFrame, host clock, alternated (the table plane estimated per frame):",
            "    with track (status %s, the volume holding the earlier frames)   %s" % (tsdf.TRACK_STATUS[status], fmt(sorted(times["track"]))),
            "    with volume (a one-view MultiView, the volume reset per frame)  %s" % fmt(sorted(times["volume"])),
            "    track - volume  %+.3f ms = %+.2f%%" % (a - b, 100.0 * (a - b) / b)]


def main():
    import numpy as np
    import torch
    from regnet_for_3d_grasping_amd import depth_frame, registration, tsdf
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "tsdf_raycast.txt"))
    args = ap.parse_args()
    mv, views = scene()
    params = tsdf.TsdfParams(origin=ORIGIN)
    track = tsdf.TrackParams(near=0.5, far=1.5)
    vol = tsdf.Volume(params, DEV)
    for view, pose in zip(views, mv.poses):
        vol.integrate(view, pose)
    k = views[0][4]
    step = params.trunc / 2
    n_steps = tsdf.ray_steps(track.near, track.far, step)
    lines = ["%s, torch %s" % (torch.cuda.get_device_name(0), torch.__version__),
             "volume %d x %d x %d voxels of %g m at %s, trunc %g m, two rendered views integrated" % (
                 params.dims + (params.voxel, ORIGIN, params.trunc)),
             "raycast %d x %d from the first view's pose, near %g m, far %g m, step %g m: %d samples per ray at most" % (
                 WIDTH, HEIGHT, track.near, track.far, step, n_steps)]
    med = statistics.median
    base = None
    for colour in (True, False):
        for clip in (True, False):
            run = lambda: vol.raycast(mv.poses[0], k, WIDTH, HEIGHT, track.near, track.far, step, colour=colour, clip=clip)  # noqa: E731
            counts = run().counts.cpu().numpy().tolist()
            t = timed(run, 3, 20)
            base = med(t) if base is None else base
            lines.append("    colour %-5s clip %-5s %s = %.2f x the first line;  no surface %d, back face %d, hit %d, hit without normal %d" % (
                (colour, clip, fmt(t), med(t) / base) + tuple(counts)))
    # the samples and corner loads, counted; and the same depth image by torch ops
    first, last = clip_range(mv.poses[0], k, WIDTH, HEIGHT, track.near, step, n_steps, params.origin, params.voxel, params.dims)
    depth, counted = torch_march(vol, mv.poses[0], k, WIDTH, HEIGHT, track.near, step, n_steps, first, last)
    visited, clipped, inside, known = (int(c) for c in counted)
    rays = WIDTH * HEIGHT
    lines.append("    counted: without the clip the rays visit %.1f M samples until they end (%.1f per ray of %d); with it %.1f M (%.1f "
                 "per ray); %.1f M of those lie inside the box and load 8 W each, %.1f M are known and load 8 D more: %.0f M "
                 "four-byte loads, %.1f per ray (counts, not traffic; the normals' and colours' samples at the %d hits not counted)" % (
                     visited / 1e6, visited / rays, n_steps, clipped / 1e6, clipped / rays, inside / 1e6, known / 1e6,
                     8 * (inside + known) / 1e6, 8 * (inside + known) / rays, counts[2] + counts[3]))
    view = vol.raycast(mv.poses[0], k, WIDTH, HEIGHT, track.near, track.far, step, colour=False)
    both = torch.isfinite(depth) & torch.isfinite(view.xyz[:, 2])
    lines.append("    the same depth image by torch ops (grid_sample over D and the observed mask, a Python loop over %d samples, no "
                 "normals, no colour)  %s;  %d of %d hits shared, depths apart by at most %.2g m" % (
                     n_steps, fmt(timed(lambda: torch_march(vol, mv.poses[0], k, WIDTH, HEIGHT, track.near, step, n_steps), 1, 5)),
                     int(both.sum()), counts[2] + counts[3], float((depth - view.xyz[:, 2])[both].abs().max())))
    # one tracked frame: the second view after the first, from the first view's pose as the guess is the last pose
    tracker = tsdf.Tracker(track_params=track, volume=vol)
    tracker.reset(mv.poses[0])
    tracker.track(views[0])
    before = vol.data.clone()

    def again():
        vol.data.copy_(before)
        tracker.pose, tracker.frames = np.array(mv.poses[0], dtype=np.float64), 1
    result = tracker.track(views[1], guess=mv.poses[1])
    lines.append("track: the second view registered against the model view from its given pose: %s, %d iterations, %d pairs, rms %.3g -> "
                 "%.3g m, moved %.3g m / %.3g rad" % ((result.status, result.report["iterations"], result.report["pairs"],
                                                       result.report["rms_first"], result.report["rms_last"])
                                                      + tsdf.relative_motion(result.report["pose"])))
    walls = []
    for _ in range(10):
        again()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        tracker.track(views[1], guess=mv.poses[1])
        torch.cuda.synchronize()
        walls.append((time.perf_counter() - t0) * 1e3)
    lines.append("    one track() call, wall clock, cloud already on the device   %s" % fmt(sorted(walls)))
    again()
    icp = track.icp_params()
    xyz = views[1][0]
    model = vol.raycast(mv.poses[1], k, WIDTH, HEIGHT, track.near, track.far, track.step, colour=False)
    target = model.target(icp, max_source=int(xyz.shape[0]))
    lines.append("    to_cloud                          %s" % fmt(timed(lambda: depth_frame.to_cloud(mv.frames[1], device=DEV), 3, 20)))
    lines.append("    raycast, no colour                %s" % fmt(timed(
        lambda: vol.raycast(mv.poses[1], k, WIDTH, HEIGHT, track.near, track.far, track.step, colour=False), 3, 20)))
    lines.append("    registration, %2d steps enqueued   %s" % (icp.iterations, fmt(timed(
        lambda: registration.icp(xyz, target, None, icp), 3, 20))))
    reg = registration.icp(xyz, target, None, icp)
    both = torch.cat([reg.state, model.counts.view(torch.uint8)])
    torch.cuda.synchronize()
    reads = []
    for _ in range(20):
        t0 = time.perf_counter()
        both.cpu()
        reads.append((time.perf_counter() - t0) * 1e3)
    lines.append("    the 1168-byte read, wall clock    %s" % fmt(sorted(reads)))
    lines.append("    integrate                         %s" % fmt(timed(lambda: vol.integrate(views[1], mv.poses[1]), 3, 20)))
    del tracker, vol, before, model, target, reg
    torch.cuda.empty_cache()
    lines += detect_lines(mv)
    text = "\n".join(lines) + "\n"
    print(text)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
