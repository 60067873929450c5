"""Projective against nearest association on the MI355X (registration.py, csrc/icp.hip, csrc/depth.hip) -> profiles/icp_projective.txt.

Both modes in the same run, on scripts/bench_icp.py's two rendered 640 x 480 views with the second camera's pose off by half a
degree and 4 mm.  Two steps, each a fresh child process under its own time limit; the driver stops at the first that fails:
  kernels  one step (two launches) of either mode at strides 1 and 3, alternated; ``depth_frame.normals`` against
           ``eval_collision.estimate_normals``; a whole registration of either mode (target preparation with its normals and
           the enqueued steps); the final pose error and rms of nearest mode and of projective mode with "image" and with "fit"
           normals, the normal gate off and at 30 degrees.  HIP-event times.
  detect   one GraspDetector.detect of the two views without ``register`` and with it in either mode, alternated.
Warm-up first, then the median of repeated runs with their min / max.

    python scripts/bench_icp_projective.py [--out profiles/icp_projective.txt]
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
from bench_grasp_nms import fmt, timed  # noqa: E402
from bench_icp import DETECT_STRIDE, DEV, FUSE, HEIGHT, ITERATIONS, MAX_DIST, WIDTH, scene  # noqa: E402

STEPS = (("kernels", 480), ("detect", 480))                      # (name, time limit in seconds)
STRIDES = (1, 3)
ANGLE = 30.0


def step_kernels(lines):
    import numpy as np
    import torch
    from regnet_for_3d_grasping_amd import depth_frame, eval_collision, fusion, registration
    from tests import icp_reference
    mv, clouds, given, truth = scene()
    source, reference = clouds[1][0], clouds[0][0]
    K = mv.frames[0].intrinsics
    near = {"max_dist": MAX_DIST, "iterations": ITERATIONS}
    proj = dict(near, association="projective")
    start = np.linalg.inv(given[0]) @ given[1]                     # source to the reference CAMERA
    target_cloud = fusion.transform_cloud(reference, given[0])
    camera = tuple(given[0][:3, 3])
    t_near = registration.prepare_target(target_cloud, near, target_camera=camera)
    t_proj = registration.prepare_projective_target(reference, WIDTH, HEIGHT, K, proj)
    finite = reference[torch.isfinite(reference).all(dim=1)].contiguous()
    image = timed(lambda: depth_frame.normals(reference, WIDTH, HEIGHT, 2, 0.02), 5, 50)
    fit = timed(lambda: eval_collision.estimate_normals(finite, (0.0, 0.0, 0.0), 0.02, 30), 2, 10)
    have = int(torch.isfinite(t_proj.normals).all(dim=1).sum())
    lines.append("normals of one %d x %d view: depth_frame.normals (step 2, jump 0.02 m; %d of %d finite rows get one)  %s;  "
                 "estimate_normals on the %d finite rows (radius 0.02 m, 30 neighbours)  %s" % (
                     WIDTH, HEIGHT, have, int(finite.shape[0]), fmt(image), int(finite.shape[0]), fmt(fit)))
    for stride in STRIDES:
        modes = (("nearest", dict(near, stride=stride), t_near, given[1], None),
                 ("projective", dict(proj, stride=stride), t_proj, start, None),
                 ("projective, gate %g deg" % ANGLE, dict(proj, stride=stride, normal_angle=ANGLE), t_proj, start,
                  depth_frame.normals(source, WIDTH, HEIGHT, 2, 0.02)))
        runs, results = [], {}
        for name, params, target, init, sn in modes:
            fresh = torch.from_numpy(registration.initial_state(init, params)).to(DEV)
            state = fresh.clone()

            def one(params=params, target=target, state=state, fresh=fresh, sn=sn):
                state.copy_(fresh)                                     # (a 1152-byte copy: the step must find RUNNING)
                registration.step(source, target, state, params, source_normals=sn)
            runs.append((name, one, state))
            results[name] = []
        for _ in range(5):                                             # alternated: every mode sees the same neighbours
            for name, one, _ in runs:
                results[name] += timed(one, 2, 10)
        copy = timed(lambda: runs[0][2].copy_(runs[0][2]), 5, 50)
        for name, one, state in runs:
            pairs = int(registration.decode_state(state.cpu().numpy())["pairs"])
            lines.append("step  stride %d, %-24s %d visited rows, %d pairs  %s  (of it a state copy %.3f ms)" % (
                stride, name + ":", -(-int(source.shape[0]) // stride), pairs, fmt(sorted(results[name])), statistics.median(copy)))
    # a whole registration: what a caller pays from two clouds to the pose, target preparation included
    stride = DETECT_STRIDE
    whole = (("nearest", lambda: registration.icp(source, target_cloud, given[1], dict(near, stride=stride), target_camera=camera)),
             ("projective", lambda: registration.icp(
                 source, registration.prepare_projective_target(reference, WIDTH, HEIGHT, K, proj), start, dict(proj, stride=stride))),
             ("projective, gate %g deg" % ANGLE, lambda: registration.icp(
                 source, registration.prepare_projective_target(reference, WIDTH, HEIGHT, K, proj), start,
                 dict(proj, stride=stride, normal_angle=ANGLE), source_shape=(WIDTH, HEIGHT))))
    times = {name: [] for name, _ in whole}
    for _ in range(3):
        for name, fn in whole:
            times[name] += timed(fn, 1, 5)
    for name, _ in whole:
        lines.append("icp   stride %d, %-24s whole registration (target, normals, %d steps enqueued)  %s" % (
            stride, name + ":", ITERATIONS, fmt(sorted(times[name]))))
    # where each mode ends
    e_given = icp_reference.pose_distance(given[1], truth[1])
    reg = registration.icp(source, t_near, given[1], dict(near, stride=stride))
    lines.append("end   stride %d, nearest:                        %s after %d iterations, %d pairs, rms %.3g -> %.3g m, pose error "
                 "%.3g -> %.3g" % (stride, registration.STATUS_NAMES[reg.status], reg.iterations, reg.pairs, reg.rms_first,
                                   reg.rms_last, e_given, icp_reference.pose_distance(reg.pose(), truth[1])))
    for normals in ("image", "fit"):
        for angle in (None, ANGLE):
            params = dict(proj, stride=stride, normals=normals, normal_angle=angle)
            target = registration.prepare_projective_target(reference, WIDTH, HEIGHT, K, params)
            reg = registration.icp(source, target, start, params, source_shape=(WIDTH, HEIGHT))
            lines.append("end   stride %d, projective, %-5s normals, gate %-4s %s after %d iterations, %d pairs, rms %.3g -> %.3g m, "
                         "pose error %.3g -> %.3g" % (
                             stride, normals, "off:" if angle is None else "%g:" % angle, registration.STATUS_NAMES[reg.status],
                             reg.iterations, reg.pairs, reg.rms_first, reg.rms_last, e_given,
                             icp_reference.pose_distance(given[0] @ reg.pose(), truth[1])))
    return True


def step_detect(lines):
    import contextlib
    import io
    import numpy as np
    import torch
    from regnet_for_3d_grasping_amd import detect, np_random, pipeline, synthetic
    from regnet_for_3d_grasping_amd.get_regiondataset import get_grasp_allobj
    mv, _, _, _ = scene()
    score_net, region_net = pipeline.build_models(DEV)
    score_net.eval()
    region_net.eval()
    base = {"max_dist": MAX_DIST, "iterations": ITERATIONS, "stride": DETECT_STRIDE}
    detectors = (("without register (baseline)", detect.GraspDetector(score_net, region_net, fuse=FUSE)),
                 ("register, nearest", detect.GraspDetector(score_net, region_net, fuse=FUSE, register=base)),
                 ("register, projective", detect.GraspDetector(score_net, region_net, fuse=FUSE,
                                                               register=dict(base, association="projective"))),
                 ("register, projective, gate %g deg" % ANGLE, detect.GraspDetector(
                     score_net, region_net, fuse=FUSE, register=dict(base, association="projective", normal_angle=ANGLE))))
    plain = detectors[0][1]
    np.random.seed(1234)
    with np_random.deferred(), torch.no_grad():
        pc = plain.ingest(mv).pc.clone()
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
        for _, detector in detectors:
            once(detector)
    times, outs = {name: [] for name, _ in detectors}, {}
    for _ in range(10):                              # alternated: all see the same neighbours on the machine
        for name, detector in detectors:
            ms, outs[name] = once(detector)
            times[name].append(ms)
    floor = statistics.median(times[detectors[0][0]])
    lines.append("GraspDetector.detect, two %d x %d views merged at %g m, register at stride %d, host clock around the call:" % (
        WIDTH, HEIGHT, FUSE["voxel"], DETECT_STRIDE))
    for name, _ in detectors:
        out, ms = outs[name], sorted(times[name])
        extra = ""
        if "fuse_register" in out:
            extra = ";  %+.3f ms = %+.2f%% of the frame time;  status %d after %d iterations, %d merged points" % (
                statistics.median(ms) - floor, 100.0 * (statistics.median(ms) - floor) / floor, int(out["fuse_register"][1, 0]),
                int(out["fuse_register"][1, 1]), int(out["fuse_num"][0]))
        lines.append("  %-36s %s%s" % (name, fmt(ms), extra))
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
    parser.add_argument("--out", default=os.path.join(REPO, "profiles", "icp_projective.txt"))
    parser.add_argument("--step", choices=[name for name, _ in STEPS], help="(internal) run one step in this process")
    parser.add_argument("--step-out", help="(internal) where the step leaves its lines")
    args = parser.parse_args()
    if args.step:
        sys.exit(run_step(args.step, args.step_out))
    import torch
    lines = ["projective against nearest association (scripts/bench_icp_projective.py): %s, torch %s; two %d x %d views, max_dist "
             "%g m, %d steps enqueued, window 1, normal_step 2, normal_jump 0.02 m; median [min .. max] of HIP-event times unless a "
             "host clock is named; both modes in this one run" % (
                 torch.cuda.get_device_name(0) if torch.cuda.is_available() else "no GPU", torch.__version__, WIDTH, HEIGHT,
                 MAX_DIST, ITERATIONS), ""]
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
                lines += json.load(f)
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
