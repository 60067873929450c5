"""What the approach analysis costs on the MI355X (approach.analyse, csrc/approach.hip) -> profiles/grasp_approach.txt.

Two steps, each a fresh child process under its own time limit; the driver stops at the first one that fails:
  kernels  B = 4000 grasps against a cloud of N = 25 600 and N = 307 200 points: ``analyse`` without and with ``friction_deg``
           (with it: normals estimated, two passes), the kernel alone (one pass, two passes), the collision filter's kernel beside
           it (eval_collision.collision_counts), ``estimate_normals`` alone, and the same outputs by torch ops on the device, a
           chunked (B,N) formulation.
  detect   one GraspDetector.detect of the synthetic camera frame with and without ``approach``, alternated; the difference as a
           share of the frame time.
Times are HIP events (kernels step) or a host clock around a call that ends in a download (detect step): warm-up first, then
the median of repeated runs with their min / max.  No time is gated.

    python scripts/bench_approach.py [--out profiles/grasp_approach.txt]
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
BOUNDS = (0.5, -0.5, 1.0, 0.5, -0.5)            # the synthetic table with room to spare (tests/test_gpu_detect.py)
B = 4000
DEPTH, WIDTH = 0.06, 0.08


def scene_and_grasps(n, seed):
    """synthetic.make_batch's scene with ``n`` points and B grasps centred on seeded points of it, random closing axes and angles."""
    import numpy as np
    from regnet_for_3d_grasping_amd import synthetic
    points = synthetic.make_batch(1000, 1, n)[0][:, :3].numpy().astype(np.float32)
    rng = np.random.default_rng(seed)
    grasp = np.zeros((B, 8), dtype=np.float32)
    grasp[:, :3] = points[rng.integers(0, n, B)] + rng.normal(0.0, 0.01, (B, 3))
    grasp[:, 3:6] = rng.standard_normal((B, 3))
    grasp[:, 6] = rng.uniform(-3.0, 3.0, B)
    grasp[:, 7] = rng.uniform(0.0, 1.0, B)
    return points, grasp


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


def torch_formulation(points, normals, T, box, standoff, contact_depth, cos_fric, chunk_elems=1 << 25):
    """The same outputs by torch ops on the device: (chunk, N) coordinate matrices, masks, masked min / max and counts."""
    import torch
    x_lo, x_hi, _, ht, hw, hs, back_x = box
    inf = float("inf")
    n = points.shape[0]
    step = max(1, chunk_elems // max(n, 1))
    P = points.t().contiguous()
    counts, values = [], []
    for s in range(0, T.shape[0], step):
        t = T[s:s + step]
        x, y, z = (t[:, r, :3] @ P + t[:, r, 3:4] for r in range(3))
        section = (z < ht) & (z > -ht) & (y < hw) & (y > -hw)
        inner = section & (y < hs) & (y > -hs)
        close = (x > x_lo) & (x < x_hi)
        region = inner & close
        hand = (section & close & (x < back_x)).sum(1) + (section & close & ((y > hs) | (y < -hs))).sum(1)
        front = torch.where(inner, back_x, x_hi)
        blocker = section & (x < front) & (x > x_lo - standoff)
        s_min = torch.where(blocker, (x_lo - x).clamp(min=0.0), inf).amin(1)
        y_min = torch.where(region, y, inf).amin(1)
        y_max = torch.where(region, y, -inf).amax(1)
        x_min = torch.where(region, x, inf).amin(1)
        cols = [region.sum(1), blocker.sum(1), hand]
        if normals is not None:
            band = torch.minimum((y_max - y_min) / 3.0, torch.full_like(y_max, contact_depth))
            ok = (t[:, 1, :3] @ normals.t()).abs() >= cos_fric
            left, right = region & (y > (y_max - band)[:, None]), region & (y < (y_min + band)[:, None])
            cols += [left.sum(1), (left & ok).sum(1), right.sum(1), (right & ok).sum(1)]
        counts.append(torch.stack(cols, 1))
        values.append(torch.stack((y_min, y_max, s_min.clamp(max=standoff), x_min), 1))
    return torch.cat(counts), torch.cat(values)


def step_kernels(lines):
    import math
    import torch
    from regnet_for_3d_grasping_amd import _lib, approach, eval_collision
    standoff, contact_depth, cos_fric = 0.10, eval_collision.NEIGHBOR_DEPTH, math.cos(math.radians(30.0))
    for n in (25600, 307200):
        host_points, host_grasp = scene_and_grasps(n, 7 + n)
        points, grasp = torch.from_numpy(host_points).to(DEV), torch.from_numpy(host_grasp).to(DEV)
        frame, center = eval_collision.grasp_frames(grasp)
        T = eval_collision.global_to_local(frame, center).contiguous()
        normals = eval_collision.estimate_normals(points)
        box, _ = eval_collision._box_args(DEPTH, WIDTH, B, points.device)
        counts = torch.empty((B, 8), dtype=torch.int32, device=DEV)
        values = torch.empty((B, 4), dtype=torch.float32, device=DEV)

        def kernel(nrm):
            n_args = (None, 0, 0) if nrm is None else (nrm.data_ptr(), nrm.stride(0), nrm.stride(1))
            _lib.call("regnet_grasp_approach_f32", points, points.data_ptr(), points.stride(0), points.stride(1), *n_args, n,
                      T.data_ptr(), B, *box, standoff, contact_depth, cos_fric, counts.data_ptr(), values.data_ptr())

        plain = timed(lambda: approach.analyse(points, grasp, DEPTH, WIDTH), 3, 20)
        friction = timed(lambda: approach.analyse(points, grasp, DEPTH, WIDTH, {"friction_deg": 30.0}), 3, 20)
        one_pass = timed(lambda: kernel(None), 3, 20)
        two_pass = timed(lambda: kernel(normals), 3, 20)
        collision = timed(lambda: eval_collision.collision_counts(points, T, DEPTH, WIDTH), 3, 20)
        estimate = timed(lambda: eval_collision.estimate_normals(points), 3, 20)
        base1 = timed(lambda: torch_formulation(points, None, T, box, standoff, contact_depth, cos_fric), 1, 3)
        base2 = timed(lambda: torch_formulation(points, normals, T, box, standoff, contact_depth, cos_fric), 1, 3)
        kernel(normals)
        got = counts.clone()
        want, _ = torch_formulation(points, normals, T, box, standoff, contact_depth, cos_fric)
        differ = int((got[:, :7] != want.to(torch.int32)).any(1).sum())
        free = int((values[:, 2] >= standoff).sum())
        lines.append("B = %d grasps, N = %d points: %d grasps with the whole standoff free, %d with points between the fingers" % (
            B, n, free, int((got[:, 0] > 0).sum())))
        lines.append("    analyse, no friction angle           %s" % fmt(plain))
        lines.append("    analyse, friction_deg = 30           %s" % fmt(friction))
        lines.append("    the kernel alone, pass 1             %s" % fmt(one_pass))
        lines.append("    the kernel alone, both passes        %s" % fmt(two_pass))
        lines.append("    collision filter's kernel beside it  %s   -> pass 1 costs %.2fx of it" % (
            fmt(collision), statistics.median(one_pass) / statistics.median(collision)))
        lines.append("    estimate_normals alone               %s" % fmt(estimate))
        lines.append("    torch ops, chunked (B,N), pass 1     %s   -> the kernel is %.1fx faster" % (
            fmt(base1), statistics.median(base1) / statistics.median(one_pass)))
        lines.append("    torch ops, chunked (B,N), both       %s   -> the kernel is %.1fx faster" % (
            fmt(base2), statistics.median(base2) / statistics.median(two_pass)))
        lines.append("    (grasps whose counts differ from the torch formulation's, whose matmul rounds otherwise: %d of %d)" % (differ, B))
    return True


def camera_frame():
    """synthetic.make_batch(1000, 1)'s scene lifted into camera coordinates, colours on the 8-bit grid of a PCD file."""
    import numpy as np
    from regnet_for_3d_grasping_amd import ingest, synthetic
    scene = synthetic.make_batch(1000, 1, 25600)[0].numpy().astype(np.float64)
    Tinv = np.linalg.inv(ingest.table_frame_transform())
    return scene[:, :3] @ Tinv[:3, :3].T + Tinv[:3, 3], np.rint(scene[:, 3:6] * 255.0) / 255.0


def step_detect(lines):
    import numpy as np
    import torch
    from regnet_for_3d_grasping_amd import detect, pipeline, synthetic
    from regnet_for_3d_grasping_amd.get_regiondataset import get_grasp_allobj
    frame = camera_frame()
    score_net, region_net = pipeline.build_models(DEV)
    score_net.eval()
    region_net.eval()
    detectors = {"plain": detect.GraspDetector(score_net, region_net, bounds=BOUNDS),
                 "approach": detect.GraspDetector(score_net, region_net, bounds=BOUNDS, approach={}),
                 "friction": detect.GraspDetector(score_net, region_net, bounds=BOUNDS, approach={"friction_deg": 30.0})}
    np.random.seed(1234)
    pc = detectors["plain"].ingest(frame).pc
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
        for detector in detectors.values():
            once(detector)
    times = {name: [] for name in detectors}
    for _ in range(15):                              # alternated: all see the same neighbours on the machine
        for name, detector in detectors.items():
            ms, out = once(detector)
            times[name].append(ms)
    a = sorted(times["plain"])
    lines.append("GraspDetector.detect, synthetic camera frame (25600 points): %d grasps in grasp_stage3 analysed" % len(out["grasp_stage3"]))
    lines.append("    without approach                     %s" % fmt(a))
    for name, label in (("approach", "with approach                        "), ("friction", "with approach, friction_deg = 30     ")):
        b = sorted(times[name])
        diff = statistics.median(b) - statistics.median(a)
        lines.append("    %s%s" % (label, fmt(b)))
        lines.append("        difference of the medians        %+9.3f ms = %+.2f%% of the frame time" % (diff, 100.0 * diff / statistics.median(a)))
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
    parser.add_argument("--out", default=os.path.join(REPO, "profiles", "grasp_approach.txt"))
    parser.add_argument("--step", choices=[name for name, _ in STEPS], help="(internal) run one step in this process")
    parser.add_argument("--step-out", help="(internal) where the step leaves its lines")
    args = parser.parse_args()
    if args.step:
        sys.exit(run_step(args.step, args.step_out))
    import torch
    lines = ["approach analysis on the device (scripts/bench_approach.py): %s, torch %s" % (
        torch.cuda.get_device_name(0) if torch.cuda.is_available() else "no GPU", torch.__version__),
        "gripper 8 cm x 6 cm, standoff 0.10 m, contact depth 5 mm; seeded grasps on synthetic.make_batch's scene; median of HIP-event times", ""]
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
