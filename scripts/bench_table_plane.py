"""What the table-plane estimate costs on the MI355X (table_plane.estimate_plane, csrc/plane.hip) -> profiles/table_plane.txt.

Two steps, each a fresh child process under its own time limit; the driver stops at the first one that fails:
  kernels  estimate_plane on the seeded 640 x 480 synthetic frame (tests/plane_reference.synthetic_frame: table, floor, four
           boxes, 1.5 mm noise, 30 % holes) at 1024 and 4096 hypotheses: the whole call (four launches + the 96-byte read), the
           four launches without the read, and each kernel on its own; the count kernel's share of its VALU bound; against the
           plain torch formulation on the device: a (H,3) @ (3,M) product, compare, sum, argmax (given the same hypotheses).
  detect   one GraspDetector.detect of that frame with ``transform={"range": ...}`` (estimated per frame) against the same
           detector with the estimated transform given explicitly -- the path without this feature --, alternated; the
           difference as a share of the frame time.
Times are HIP events (kernels step) or a host clock around a call that ends in a download (detect step): warm-up first, then
the median of repeated runs with their min / max.

    python scripts/bench_table_plane.py [--out profiles/table_plane.txt]
"""
import argparse
import contextlib
import io
import json
import os
import statistics
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)
DEV = "cuda:0"
STEPS = (("kernels", 420), ("detect", 420))     # (name, time limit in seconds)
RANGE = (0.5, 1.2)
VALU_OPS_PER_TEST = 10                          # 3 subtractions, 4 products, 2 sums, 1 compare
VALU_LANES_PER_CLOCK = 256 * 4 * 32             # 256 CUs x 4 SIMDs x 32 lanes
CLOCK_HZ = 2.4e9


def timed(fn, warmup, repeats):
    """-> sorted HIP-event times of ``fn()`` in milliseconds (each ends when the stream has passed the call)."""
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(repeats):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        fn()
        stop.record()
        stop.synchronize()
        times.append(start.elapsed_time(stop))
    return sorted(times)


def fmt(times):
    return "%9.3f ms  (min %.3f, max %.3f, %d runs)" % (statistics.median(times), times[0], times[-1], len(times))


def torch_formulation(xyz, table, threshold):
    """The baseline: every hypothesis against every point as one product, on the device -> (winner, count) tensors."""
    import torch
    finite = torch.isfinite(xyz).all(dim=1)
    p = torch.where(finite[:, None], xyz, torch.full_like(xyz, float("nan")))
    n, p0, nn = table[:, 0:3], table[:, 3:6], table[:, 6]
    s = n @ p.t() - (n * p0).sum(dim=1)[:, None]
    inlier = s * s <= (threshold * threshold) * nn[:, None]
    counts = inlier.sum(dim=1)
    counts = torch.where(table[:, 7] == 2.0, counts, torch.full_like(counts, -1))
    winner = torch.argmax(counts)
    return winner, counts[winner]


def step_kernels(lines):
    import torch
    from regnet_for_3d_grasping_amd import table_plane
    from tests import plane_reference as ref
    xyz = torch.from_numpy(ref.synthetic_frame()[0]).to(DEV)
    M = int(xyz.shape[0])
    for H in (1024, 4096):
        out = table_plane.estimate_device(xyz, hypotheses=H, range=RANGE)
        plane = table_plane.estimate_plane(xyz, hypotheses=H, range=RANGE)
        lines.append("H = %4d  M = %d (%d finite): hypothesis %d, %d inliers, rms %.3f mm" % (
            H, M, int(torch.isfinite(xyz).all(dim=1).sum()), plane.hypothesis, plane.inliers, plane.rms * 1e3))
        whole = timed(lambda: table_plane.estimate_plane(xyz, hypotheses=H, range=RANGE), 5, 30)
        four = timed(lambda: table_plane.estimate_device(xyz, hypotheses=H, range=RANGE, out=out), 5, 30)
        lines.append("    estimate_plane, whole call          %s" % fmt(whole))
        lines.append("    the four kernels, no read           %s" % fmt(four))
        for name, stage in (("plane_hypotheses_kernel", 1), ("plane_count_kernel", 2), ("plane_select_kernel", 4),
                            ("plane_moments_kernel", 8)):
            table_plane.estimate_device(xyz, hypotheses=H, range=RANGE, out=out)          # the inputs of every stage, fresh
            times = timed(lambda: table_plane.estimate_device(xyz, hypotheses=H, range=RANGE, out=out, stages=stage), 5, 30)
            lines.append("        %-28s    %s" % (name, fmt(times)))
            if stage == 2:
                bound = M * H * VALU_OPS_PER_TEST / (VALU_LANES_PER_CLOCK * CLOCK_HZ) * 1e3
                lines.append("        its VALU bound (%d ops per test, %d lanes, 2.4 GHz): %.3f ms -> %.0f%% of the bound's rate" % (
                    VALU_OPS_PER_TEST, VALU_LANES_PER_CLOCK, bound, 100.0 * bound / statistics.median(times)))
        table = out[1].hypotheses.clone()
        winner, count = torch_formulation(xyz, table, 0.005)
        base = timed(lambda: torch_formulation(xyz, table, 0.005), 2, 10)
        lines.append("    torch formulation (product, compare, sum, argmax; hypotheses given): winner %d, %d inliers" % (
            int(winner), int(count)))
        ratio = statistics.median(base) / statistics.median(four)
        lines.append("                                        %s   -> the four kernels are %.1fx %s" % (
            fmt(base), ratio if ratio >= 1.0 else 1.0 / ratio, "faster" if ratio >= 1.0 else "SLOWER"))
    return True


def step_detect(lines):
    import numpy as np
    import torch
    from regnet_for_3d_grasping_amd import detect, np_random, pipeline, synthetic
    from regnet_for_3d_grasping_amd.get_regiondataset import get_grasp_allobj
    from tests import plane_reference as ref
    frame = ref.synthetic_frame(dtype=np.float64)
    score_net, region_net = pipeline.build_models(DEV)
    score_net.eval()
    region_net.eval()
    auto = detect.GraspDetector(score_net, region_net, transform={"range": RANGE})
    np.random.seed(1234)
    with np_random.deferred(), torch.no_grad():
        pc = auto.ingest(frame).pc.clone()
    explicit = detect.GraspDetector(score_net, region_net, transform=auto.table[0])
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
        out = detector.detect(frame)
        return (time.perf_counter() - t0) * 1e3, out
    for _ in range(3):
        once(explicit)
        once(auto)
    times = {"explicit": [], "auto": []}
    for _ in range(15):                              # alternated: both see the same neighbours on the machine
        times["explicit"].append(once(explicit)[0])
        ms, out = once(auto)
        times["auto"].append(ms)
    a, b = sorted(times["explicit"]), sorted(times["auto"])
    diff = statistics.median(b) - statistics.median(a)
    lines.append("GraspDetector.detect, the 640 x 480 float64 frame from the host: %d points kept, %d grasps in grasp_stage3" % (
        len(out["points"]), len(out["grasp_stage3"])))
    lines.append("    transform given (as before)     %s" % fmt(a))
    lines.append("    transform estimated per frame   %s" % fmt(b))
    lines.append("    difference of the medians       %+9.3f ms = %+.2f%% of the frame time" % (diff, 100.0 * diff / statistics.median(a)))
    return True


def run_step(name, path):
    import torch
    assert torch.cuda.is_available(), "this measurement needs the MI355X"
    lines = []
    ok = {"kernels": step_kernels, "detect": step_detect}[name](lines)
    with open(path, "w") as f:
        json.dump(lines, f)
    return 0 if ok else 1


def main():
    parser = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    parser.add_argument("--out", default=os.path.join(REPO, "profiles", "table_plane.txt"))
    parser.add_argument("--step", choices=[name for name, _ in STEPS], help="(internal) run one step in this process")
    parser.add_argument("--step-out", help="(internal) where the step leaves its lines")
    args = parser.parse_args()
    if args.step:
        sys.exit(run_step(args.step, args.step_out))
    import torch
    lines = ["table plane on the device (scripts/bench_table_plane.py): %s, torch %s" % (
        torch.cuda.get_device_name(0) if torch.cuda.is_available() else "no GPU", torch.__version__),
        "threshold 0.005 m, range %.1f-%.1f m, seed 0; seeded 640 x 480 frame with 30 %% holes; median of HIP-event times" % RANGE, ""]
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
