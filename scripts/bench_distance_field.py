"""What the distance field of the TSDF volume costs on the MI355X (tsdf.Volume.distance_field, csrc/edt.hip)
-> profiles/distance_field.txt.

Two steps, each a fresh child process under its own time limit; the driver stops at the first one that fails:
  field    the rendered two-view volume of scripts/bench_tsdf.py (320^3 voxels of 2 mm), both modes: the three line passes singly
           (each on the state the pass before it left, restored outside the timed region), the whole call with and without
           ``nearest``, ``query`` of 10^6 points, the margin kernel at B = 16 and B = 4000 beside
           regnet_grasp_approach_volume_f32 on the same grasps, and the host route -- download, scipy's
           ``distance_transform_edt`` -- on the host clock.  Beside every pass stands its byte bound: the words it must read and
           write over 8 TB/s, a count and not measured traffic.
  detect   one GraspDetector.detect of the two-view MultiView in volume space without and with ``field``, alternated.
Times are HIP events (field step) or a host clock around a call that ends in a download (detect step, host route): warm-up
first, then the median of repeated runs with their min / max.  No time is gated.

    python scripts/bench_distance_field.py [--out profiles/distance_field.txt]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_outliers import fmt, timed  # noqa: E402
from bench_tsdf import ORIGIN, scene  # noqa: E402

DEV = "cuda:0"
STEPS = (("field", 540), ("detect", 420))       # (name, time limit in seconds)
DEPTH, WIDTH = 0.06, 0.08
STANDOFF = 0.10
HBM = 8.0e12                                    # bytes per second: the byte bound's denominator


def timed_after(restore, fn, warmup, repeats):
    """``timed`` with ``restore()`` run before every ``fn()``, outside the pair of events."""
    import torch
    times = []
    for r in range(warmup + repeats):
        restore()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        if r >= warmup:
            times.append(a.elapsed_time(b))
    return sorted(times)


def step_field(lines):
    import numpy as np
    import torch
    from regnet_for_3d_grasping_amd import _lib, approach, eval_collision, tsdf
    mv, views = scene()
    params = tsdf.TsdfParams(origin=ORIGIN)
    vol = tsdf.Volume(params, DEV)
    for v in (0, 1):
        vol.integrate(views[v], mv.poses[v])
    surface = vol.extract()
    k, _, observed = surface.check()
    nx, ny, nz = params.dims
    n = nx * ny * nz
    lines.append("volume %d x %d x %d voxels of %g m, two views integrated: %d observed voxels, %d surface rows" % (
        params.dims + (params.voxel, observed, k)))
    med = statistics.median
    host_cloud = surface.xyz[:k].cpu().numpy()
    for mode in tsdf.FIELD_MODES:
        outside = mode == "solid_or_unseen"
        field = vol.distance_field(mode, nearest=True)
        obstacles = int((field.dist2 == 0).sum())
        finite = field.dist2[field.dist2 < tsdf.EDT_NONE]
        lines.append("mode %s, outside %d: %d obstacle voxels (%.2f%%), largest distance %.1f voxels" % (
            mode, outside, obstacles, 100.0 * obstacles / n, float(finite.max()) ** 0.5 if finite.numel() else float("inf")))
        for nearest in (False, True):
            d2 = torch.empty((n,), dtype=torch.int32, device=DEV)
            near = torch.empty((n,), dtype=torch.int32, device=DEV) if nearest else None
            saved = [None, None]

            def one(p):
                _lib.call("regnet_tsdf_edt_pass", vol.data, vol.data.data_ptr(), nx, ny, nz, float(params.trunc),
                          int(params.min_weight), 0.0, tsdf.FIELD_MODES.index(mode), int(outside), p, d2.data_ptr(),
                          None if near is None else near.data_ptr())

            def restore():
                if saved[0] is not None:
                    d2.copy_(saved[0])
                    if nearest:
                        near.copy_(saved[1])

            words = 2 if nearest else 1
            # pass x reads W and (where observed) D and writes the planes; y and z read and write the planes
            bounds = [(2 + words) * 4 * n / HBM * 1e3, 2 * words * 4 * n / HBM * 1e3, 2 * words * 4 * n / HBM * 1e3]
            lines.append("  %s nearest (%d B per voxel), tile of the y / z pass: %d lines" % (
                "with" if nearest else "without", 4 * words, int(_lib.lib.regnet_edt_tile(ny, int(nearest)))))
            total = 0.0
            for p, name in enumerate("xyz"):
                t = timed_after(restore, lambda: one(p), 2, 10)
                total += med(t)
                lines.append("    pass %s                                    %s   byte bound %.3f ms: %.1fx of it" % (
                    name, fmt(t), bounds[p], med(t) / bounds[p]))
                restore()
                one(p)
                saved = [d2.clone(), near.clone() if nearest else None]
            t = timed(lambda: vol.distance_field(mode, nearest=nearest, out=field), 2, 10)
            lines.append("    Volume.distance_field (three launches)    %s   byte bound %.3f ms; the passes singly add up to %.3f ms" % (
                fmt(t), sum(bounds), total))
        field = vol.distance_field(mode, nearest=True)
        rng = np.random.default_rng(3)
        lo = np.asarray(ORIGIN)
        points = torch.from_numpy(rng.uniform(lo, lo + np.asarray(params.dims) * params.voxel, (1000000, 3)).astype(np.float32)).to(DEV)
        t = timed(lambda: field.query(points), 2, 10)
        t_near = timed(lambda: field.query(points, nearest=True), 2, 10)
        lines.append("  query of 10^6 uniform points                  %s   with nearest_xyz %s" % (fmt(t), fmt(t_near)))
        t = timed(lambda: field.metres(), 2, 10)
        lines.append("  metres() of the whole field                   %s" % fmt(t))
        for B in (16, 4000):
            grasp = np.zeros((B, 8), dtype=np.float32)
            grng = np.random.default_rng(11)
            grasp[:, :3] = host_cloud[grng.integers(0, k, B)] + grng.normal(0.0, 0.01, (B, 3))
            grasp[:, 3:6] = grng.standard_normal((B, 3))
            grasp[:, 6] = grng.uniform(-3.0, 3.0, B)
            grasp = torch.from_numpy(grasp).to(DEV)
            res = approach.analyse_volume(vol, grasp, DEPTH, WIDTH, {"standoff": STANDOFF, "space": "volume"}, field=field)
            box, _ = eval_collision._box_args(DEPTH, WIDTH, B, grasp.device)
            counts, values = torch.empty_like(res.counts), torch.empty_like(res.values)
            margins, mcounts = torch.empty_like(res.margins), torch.empty_like(res.margin_counts)

            def classify():
                _lib.call("regnet_grasp_approach_volume_f32", vol.data, vol.data.data_ptr(), nx, ny, nz, vol.origin.ctypes.data,
                          float(params.voxel), float(params.trunc), int(params.min_weight), 0.0, res.L.data_ptr(), B, *box, STANDOFF,
                          float(params.voxel), DEPTH, counts.data_ptr(), values.data_ptr())

            def margin():
                _lib.call("regnet_grasp_margin_volume_f32", field.dist2, field.dist2.data_ptr(), nx, ny, nz, vol.origin.ctypes.data,
                          float(params.voxel), int(outside), res.L.data_ptr(), B, *box, STANDOFF, float(params.voxel), DEPTH,
                          margins.data_ptr(), mcounts.data_ptr())

            t_c, t_m = timed(classify, 3, 20), timed(margin, 3, 20)
            hand = res.margin_hand
            lines.append("  B = %4d: regnet_grasp_margin_volume_f32       %s" % (B, fmt(t_m)))
            lines.append("            regnet_grasp_approach_volume_f32     %s   -> the margin kernel costs %.2fx of it" % (
                fmt(t_c), med(t_m) / med(t_c)))
            lines.append("            margin_hand: %d grasps at 0, median %.4f m, %d swept samples of %d outside the volume" % (
                int((hand == 0).sum()), float(hand.median()), int(res.margin_counts[:, 3].sum()), int(res.margin_counts[:, 2].sum())))
        try:
            from scipy import ndimage
        except ImportError:
            lines.append("  host route: scipy is not installed here, not measured")
            continue
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        mask = (field.dist2 == 0).cpu().numpy().reshape(nz, ny, nx)
        t1 = time.perf_counter()
        host = ndimage.distance_transform_edt(~mask) if mask.any() else None
        t2 = time.perf_counter()
        same = "not compared (no obstacle)"
        if host is not None and not outside:
            same = "equal to the device's dist2" if np.array_equal(np.rint(host ** 2).astype(np.int64).reshape(-1),
                                                                     field.dist2.cpu().numpy().astype(np.int64)) else "DIFFERENT"
        elif host is not None:
            same = "not compared (scipy has no outside rule)"
        lines.append("  host route, one run, host clock: download of the mask %.1f ms, scipy.ndimage.distance_transform_edt %.1f ms; %s" % (
            (t1 - t0) * 1e3, (t2 - t1) * 1e3, same))
    return True


def step_detect(lines):
    import contextlib
    import io
    import numpy as np
    import torch
    from regnet_for_3d_grasping_amd import detect, pipeline, synthetic
    from regnet_for_3d_grasping_amd.get_regiondataset import get_grasp_allobj
    mv, _ = scene()
    score_net, region_net = pipeline.build_models(DEV)
    score_net.eval()
    region_net.eval()
    detectors = {"plain": detect.GraspDetector(score_net, region_net, volume={"origin": ORIGIN}, approach={"space": "volume"}),
                 "field": detect.GraspDetector(score_net, region_net, volume={"origin": ORIGIN},
                                               approach={"space": "volume", "field": True})}
    np.random.seed(1234)
    pc = detect.GraspDetector(score_net, region_net).ingest(mv).pc
    synthetic.calibrate_score_head(score_net, pc)
    with torch.no_grad():
        feat, score, _ = score_net(pc)
    np.random.seed(41)
    g = get_grasp_allobj(pc, score, detect.TEST_PARAMS, [], True)

    def region():
        with contextlib.redirect_stdout(io.StringIO()), torch.no_grad():
            return region_net(g[3], g[5], g[2], g[4], g[0], g[1], pc, feat, detect.GRIPPER_PARAMS, None, [])
    np.random.seed(5)
    synthetic.calibrate_region_head(region_net, region)

    def once(detector):
        np.random.seed(1234)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = detector.detect(mv)
        return (time.perf_counter() - t0) * 1e3, out
    for _ in range(3):
        for detector in detectors.values():
            once(detector)
    times = {name: [] for name in detectors}
    for _ in range(15):                              # alternated: both see the same neighbours on the machine
        for name, detector in detectors.items():
            ms, out = once(detector)
            times[name].append(ms)
    a, b = sorted(times["plain"]), sorted(times["field"])
    diff = statistics.median(b) - statistics.median(a)
    lines.append("GraspDetector.detect of two 640 x 480 views through the volume, approach in volume space, host clock, %d grasps of "
                 "grasp_stage3 analysed:" % len(out["grasp_stage3"]))
    lines.append("    without the field (--approach-space volume)   %s" % fmt(a))
    lines.append("    with the field (--approach-field)             %s" % fmt(b))
    lines.append("    difference of the medians  %+9.3f ms = %+.2f%% of the frame time" % (diff, 100.0 * diff / statistics.median(a)))
    return True


def run_step(name, path):
    import torch
    assert torch.cuda.is_available(), "this measurement needs the MI355X"
    lines = []
    ok = {"field": step_field, "detect": step_detect}[name](lines)
    with open(path, "w") as f:
        json.dump(lines, f)
    return 0 if ok else 1


def main():
    parser = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    parser.add_argument("--out", default=os.path.join(REPO, "profiles", "distance_field.txt"))
    parser.add_argument("--step", choices=[name for name, _ in STEPS], help="(internal) run one step in this process")
    parser.add_argument("--step-out", help="(internal) where the step leaves its lines")
    args = parser.parse_args()
    if args.step:
        sys.exit(run_step(args.step, args.step_out))
    import torch
    lines = ["distance field of the TSDF volume (scripts/bench_distance_field.py): %s, torch %s" % (
        torch.cuda.get_device_name(0) if torch.cuda.is_available() else "no GPU", torch.__version__),
        "the two-view volume of scripts/bench_tsdf.py; gripper 8 cm x 6 cm, standoff %.2f m, step = the 2 mm voxel; median of HIP-event "
        "times unless a host clock is named; byte bound = the words a pass must read and write over 8 TB/s, a count" % STANDOFF, ""]
    status = 0
    for name, limit in STEPS:
        part = args.out + "." + name + ".json"
        try:
            status = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", name, "--step-out", part],
                                    timeout=limit).returncode
        except subprocess.TimeoutExpired:
            status = 124
        if os.path.exists(part):
            with open(part) as f:
                lines += json.load(f) + [""]
            os.remove(part)
        if status != 0:                              # nothing more is started on the GPU after a step that failed
            lines.append("step %s ended with status %d: stopped here" % (name, status))
            break
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines).rstrip() + "\n")
    print("\n".join(lines))
    sys.exit(status)


if __name__ == "__main__":
    main()
