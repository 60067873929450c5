"""What coarse-to-fine tracking costs on the MI355X (depth_frame.smooth / halve, registration.continue_state, tsdf.Tracker with
``levels`` / ``smooth``) and what it buys on the restated loop -> profiles/track_pyramid.txt.

Two parts, kept apart by the line ``MARK``:

  * the capture-range table of tests/test_depth_pyramid_reference_cpu.py (``sweep_table``): the restated loop on a rendered
    scene, no GPU (``--sweep``);
  * HIP-event times on the two rendered 640 x 480 views of scripts/bench_tsdf.py in the default volume: ``smooth``, each
    ``halve``, the three raycasts of a three-level pyramid, the registration's enqueued steps, and one ``Tracker.track`` call
    with ``levels = 3`` against ``levels = 1`` -- the single-level path as it was -- alternated in the same run, wall clock with
    a synchronise; and the launches the new path adds, counted from the contracts (``--times``, needs the GPU).

Either part leaves the other as the file has it.

    python scripts/bench_track_pyramid.py --sweep --times [--out profiles/track_pyramid.txt]
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

MARK = "---- times on the device ----"
NOT_MEASURED = "not measured: the run on the MI355X could not be made"


def sweep_lines():
    from tests import test_depth_pyramid_reference_cpu as cpu
    return cpu.sweep_table() + [
        "No row separates the two: both follow the frame up to m = 25 and both end tens of centimetres off from m = 26 on.  On this",
        "scene (large walls, point-to-plane residuals, noise-free depth) the single level's capture range is not what limits the",
        "tracker; the pyramid neither widens nor narrows it.  The feature stays opt-in."]


def launches(levels, budgets, smooth):
    """Kernel launches of the project's own entry points in one registration of the coarse-to-fine path, from their contracts:
    to_cloud 2 and raycast 2 per level, a step 2, a halving and a hand-over 1 each, the filter 1."""
    return (1 if smooth else 0) + (levels - 1) + 4 * levels + 2 * sum(budgets) + (levels - 1)


def time_lines():
    import numpy as np
    import torch
    from bench_outliers import fmt, timed
    from bench_tsdf import DEV, HEIGHT, ORIGIN, WIDTH, scene
    from regnet_for_3d_grasping_amd import depth_frame, registration, tsdf
    mv, views = scene()
    params = tsdf.TsdfParams(origin=ORIGIN)
    single = tsdf.TrackParams(near=0.5, far=1.5)
    three = tsdf.TrackParams(near=0.5, far=1.5, levels=3)
    smoothed = tsdf.TrackParams(near=0.5, far=1.5, levels=3, smooth=depth_frame.SmoothParams())
    vol = tsdf.Volume(params, DEV)
    for view, pose in zip(views, mv.poses):
        vol.integrate(view, pose)
    xyz, k = views[1][0], views[1][4]
    depth = xyz[:, 2].reshape(HEIGHT, WIDTH).contiguous()
    lines = [MARK, "%s, torch %s" % (torch.cuda.get_device_name(0), torch.__version__),
             "the second of two rendered %d x %d views against the default volume (%d^3 voxels of %g m) holding both; HIP events,"
             % (WIDTH, HEIGHT, params.dims[0], params.voxel), "median (min, max) after warm-up"]
    sp = depth_frame.SmoothParams()
    tables = torch.from_numpy(depth_frame.smooth_tables(sp)).to(DEV)
    out = torch.empty_like(depth)
    taps = (2 * sp.radius + 1) ** 2 * WIDTH * HEIGHT
    t = timed(lambda: depth_frame.smooth(depth, sp, out=out, tables=tables), 5, 30)
    lines.append("    smooth, radius %d (%.1f M taps, %.1f MB in and out)     %s" % (sp.radius, taps / 1e6, 8 * WIDTH * HEIGHT / 1e6, fmt(t)))
    pyramid = depth_frame.pyramid(depth, k, 3, three.max_dist)
    for level in (1, 2):
        src = pyramid[level - 1][0]
        dst = torch.empty_like(pyramid[level][0])
        lines.append("    halve %4d x %3d -> %3d x %3d                            %s" % (
            pyramid[level - 1][2], pyramid[level - 1][3], pyramid[level][2], pyramid[level][3],
            fmt(timed(lambda: depth_frame.halve(src, three.max_dist, out=dst), 5, 30))))
    for _, k_l, w_l, h_l in pyramid:
        lines.append("    raycast %4d x %3d, no colour                            %s" % (w_l, h_l, fmt(timed(
            lambda: vol.raycast(mv.poses[1], k_l, w_l, h_l, three.near, three.far, three.step, colour=False), 3, 20))))
    state = torch.empty((registration.STATE_BYTES,), dtype=torch.uint8, device=DEV)
    lines.append("    continue_state (one thread)                              %s" % fmt(timed(
        lambda: registration.continue_state(state.zero_(), 5), 5, 30)))
    for name, t in (("levels = 1, %d steps" % single.iterations, single), ("levels = 3, %s steps" % (three.budgets(),), three)):
        def run():
            st = torch.from_numpy(registration.initial_state(None, t.icp_params(t.levels - 1))).to(DEV)
            for level in range(t.levels - 1, -1, -1):
                z_l, k_l, w_l, h_l = pyramid[level]
                icp = t.icp_params(level) if t.pyramid() else t.icp_params()
                registration.icp(clouds[level], targets[level], None, icp, state=st)
                if level > 0:
                    registration.continue_state(st, t.budgets()[level - 1])
        clouds, targets = [], []
        for z_l, k_l, w_l, h_l in pyramid[:t.levels]:
            clouds.append(depth_frame.to_cloud(depth_frame.DepthFrame(depth=z_l, intrinsics=k_l), device=DEV)[0])
            model = vol.raycast(mv.poses[1], k_l, w_l, h_l, t.near, t.far, t.step, colour=False)
            targets.append(model.target(t.icp_params(), max_source=w_l * h_l))
        lines.append("    registration, %-28s %s" % (name, fmt(timed(run, 3, 20))))
    # one track() call each way, alternated: the volume and the pose put back before every call
    trackers = {}
    for name, t in (("levels = 1 (the path as it was)", single), ("levels = 3", three), ("levels = 3, smooth", smoothed)):
        tracker = tsdf.Tracker(track_params=t, volume=tsdf.Volume(params, DEV))
        tracker.reset(mv.poses[0])
        for view, pose in zip(views, mv.poses):
            tracker.volume.integrate(view, pose)
        trackers[name] = (tracker, tracker.volume.data.clone(), [])
    report = {}
    for j in range(12):
        for name, (tracker, before, walls) in trackers.items():
            tracker.volume.data.copy_(before)
            tracker.pose, tracker.frames = np.array(mv.poses[0], dtype=np.float64), 1
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            result = tracker.track(views[1], guess=mv.poses[1])
            torch.cuda.synchronize()
            if j >= 2:
                walls.append((time.perf_counter() - t0) * 1e3)
            report[name] = result
    lines.append("one track() call, wall clock with a synchronise, cloud already on the device, the three alternated:")
    base = statistics.median(trackers["levels = 1 (the path as it was)"][2])
    for name, (tracker, _, walls) in trackers.items():
        r, t = report[name], tracker.params
        n = 2 + 2 * t.iterations if not t.pyramid() else launches(t.levels, t.budgets(), t.smooth is not None)
        lines.append("    %-32s %s = %.2f x;  %s, %d iterations, %d pairs, rms %.3g m; %d launches of the project's kernels before the read"
                     % (name, fmt(sorted(walls)), statistics.median(walls) / base, r.status, r.report["iterations"], r.report["pairs"],
                        r.report["rms_last"], n))
    lines.append("(launches counted from the contracts: raycast 2, a step 2, to_cloud 2 per level, a halving, a hand-over and the filter 1 each;")
    lines.append(" the new path adds torch's copy of the z column, the zeroed marks and a longer concatenation before the one read)")
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "track_pyramid.txt"))
    ap.add_argument("--sweep", action="store_true", help="the capture-range table of the restated loop (no GPU)")
    ap.add_argument("--times", action="store_true", help="the times on the device")
    args = ap.parse_args()
    sweep, times = [], [MARK, NOT_MEASURED]
    if os.path.exists(args.out):
        with open(args.out) as f:
            old = f.read().split("\n")
        cut = old.index(MARK) if MARK in old else len(old)
        sweep, times = [line for line in old[:cut]], ([line for line in old[cut:] if line] or times)
        sweep = sweep[:-1] if sweep and sweep[-1] == "" else sweep
    if args.sweep:
        sweep = sweep_lines()
    if args.times:
        times = time_lines()
    text = "\n".join(sweep + times) + "\n"
    print(text)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
