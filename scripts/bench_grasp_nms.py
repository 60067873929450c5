"""What pose NMS + top-K costs on the MI355X (grasp_select.pose_nms, csrc/nms.hip) -> profiles/grasp_nms.txt.

Two steps, each a fresh child process under its own time limit; the driver stops at the first one that fails:
  kernels  pose_nms at n = 4000 and n = 16000, top_k None and 64, on seeded clustered grasps: the whole call (frames, ranking,
           two kernels, the 4-byte read of the count) and the two kernels alone, against baseline (a), the obvious torch
           formulation -- pairwise matrices by torch ops on the GPU, the mask downloaded, the greedy loop on the host.
           The step FAILS unless the whole call beats (a) at every size.
  detect   baseline (b): one GraspDetector.detect of the synthetic camera frame with and without ``select``, alternated; the
           difference as a share of the frame time.
Times are HIP events (kernels step) or a host clock around a call that ends in a download (detect step): warm-up first, then
the median of repeated runs with their min / max.

    python scripts/bench_grasp_nms.py [--out profiles/grasp_nms.txt]
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


def clustered_grasps(n, seed):
    """(n,8) float32: n // 6 cluster poses, members with jittered centres, axes and angles, a third of them half a turn about
    the approach axis away (axis_y negated), uniform scores."""
    import numpy as np
    rng = np.random.default_rng(seed)
    k = max(1, n // 6)
    member = rng.integers(0, k, n)
    center = rng.uniform(-0.3, 0.3, (k, 3))[member] + rng.normal(0.0, 0.004, (n, 3))
    axis = rng.standard_normal((k, 3))[member]
    axis = axis / np.linalg.norm(axis, axis=1, keepdims=True) + rng.normal(0.0, 0.05, (n, 3))
    axis[rng.uniform(size=n) < 0.3] *= -1.0
    angle = rng.uniform(-3.0, 3.0, k)[member] + rng.normal(0.0, 0.05, n)
    out = np.zeros((n, 8), dtype=np.float32)
    out[:, :3], out[:, 3:6], out[:, 6], out[:, 7] = center, axis, angle, rng.uniform(0.0, 1.0, n)
    return out


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


def torch_baseline(grasp, t, deg, top_k, symmetric=True):
    """Baseline (a): pairwise matrices by torch ops on the GPU, the mask downloaded, the greedy loop on the host."""
    import numpy as np
    import torch
    from regnet_for_3d_grasping_amd import eval_collision, grasp_select
    T2, C = grasp_select.thresholds(t, deg)
    frame, center = eval_collision.grasp_frames(grasp[:, :8].contiguous())
    order = grasp_select.rank_order(grasp[:, 7])
    c, F = center[order], frame[order]
    d2 = torch.cdist(c, c).square_()
    da, db, dm = (F[:, :, k] @ F[:, :, k].t() for k in range(3))
    tr = da + db + dm
    if symmetric:
        tr = torch.maximum(tr, da - db - dm)
    mask = ((d2 <= T2) & (tr >= C)).cpu().numpy()
    order = order.cpu().numpy()
    n = len(order)
    limit = n if not top_k or top_k <= 0 else top_k
    removed = np.zeros(n, dtype=bool)
    keep = []
    for i in range(n):
        if removed[i]:
            continue
        keep.append(order[i])
        if len(keep) >= limit:
            break
        removed |= mask[i]
    return np.asarray(keep, dtype=np.int64)


def step_kernels(lines):
    import torch
    from regnet_for_3d_grasping_amd import eval_collision, grasp_select
    ok = True
    for n in (4000, 16000):
        grasp = torch.from_numpy(clustered_grasps(n, 100 + n)).to(DEV)
        frame, center = eval_collision.grasp_frames(grasp)
        order = grasp_select.rank_order(grasp[:, 7])
        keep = torch.empty((n,), dtype=torch.int64, device=DEV)
        count = torch.empty((1,), dtype=torch.int32, device=DEV)
        ws = torch.empty((grasp_select.workspace_bytes(n),), dtype=torch.uint8, device=DEV)
        for top_k in (None, 64):
            whole = timed(lambda: grasp_select.pose_nms(grasp, top_k=top_k), 5, 30)
            alone = timed(lambda: grasp_select.nms_ranked(center, frame, order, top_k=top_k, keep=keep, count=count, workspace=ws),
                          5, 30)
            base = timed(lambda: torch_baseline(grasp, 0.03, 30.0, top_k), 2, 5)
            kept = int(grasp_select.pose_nms(grasp, top_k=top_k).shape[0])
            kept_base = len(torch_baseline(grasp, 0.03, 30.0, top_k))
            faster = statistics.median(whole) < statistics.median(base)
            ok = ok and faster
            lines.append("n = %5d  top_k = %-4s  kept %d (torch formulation: %d)" % (n, top_k, kept, kept_base))
            lines.append("    pose_nms, whole call            %s" % fmt(whole))
            lines.append("    the two kernels alone           %s" % fmt(alone))
            lines.append("    (a) torch ops + host greedy     %s   -> pose_nms is %.1fx faster%s" % (
                fmt(base), statistics.median(base) / statistics.median(whole), "" if faster else "   ** SLOWER: a defect **"))
    return ok


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
    plain = detect.GraspDetector(score_net, region_net, bounds=BOUNDS)
    select = detect.GraspDetector(score_net, region_net, bounds=BOUNDS, select={"top_k": 64})
    np.random.seed(1234)
    pc = plain.ingest(frame).pc
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
        once(plain)
        once(select)
    times = {"plain": [], "select": []}
    for _ in range(15):                              # alternated: both see the same neighbours on the machine
        times["plain"].append(once(plain)[0])
        ms, out = once(select)
        times["select"].append(ms)
    a, b = sorted(times["plain"]), sorted(times["select"])
    diff = statistics.median(b) - statistics.median(a)
    lines.append("GraspDetector.detect, synthetic camera frame (25600 points): %d grasps in grasp_stage3 -> %d selected" % (
        len(out["grasp_stage3"]), len(out["grasp_selected"])))
    lines.append("    (b) without select              %s" % fmt(a))
    lines.append("        with select (top_k 64)      %s" % fmt(b))
    lines.append("        difference of the medians   %+9.3f ms = %+.2f%% of the frame time" % (diff, 100.0 * diff / statistics.median(a)))
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
    parser.add_argument("--out", default=os.path.join(REPO, "profiles", "grasp_nms.txt"))
    parser.add_argument("--step", choices=[name for name, _ in STEPS], help="(internal) run one step in this process")
    parser.add_argument("--step-out", help="(internal) where the step leaves its lines")
    args = parser.parse_args()
    if args.step:
        sys.exit(run_step(args.step, args.step_out))
    import torch
    lines = ["pose NMS + top-K on the device (scripts/bench_grasp_nms.py): %s, torch %s" % (
        torch.cuda.get_device_name(0) if torch.cuda.is_available() else "no GPU", torch.__version__),
        "thresholds 0.03 m / 30 deg, symmetric; clustered seeded grasps (n // 6 clusters); median of HIP-event times", ""]
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
