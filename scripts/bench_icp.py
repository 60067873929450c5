"""What pose refinement costs on the MI355X (registration.py, csrc/icp.hip) -> profiles/icp_register.txt.

Three steps, each a fresh child process under its own time limit; the driver stops at the first one that fails:
  kernels  two 640 x 480 views (tests/fuse_reference.two_view_scene, deprojected by to_cloud), the second camera's pose off by half
           a degree and 4 mm, registered onto the first at stride 1, 4 and 3 (4 divides the width: every fourth pixel column of
           the organised cloud and nothing between; 3 does not): one step (two launches) on a prepared target, the target's
           preparation without and with its normals, and a whole registration (prepare + normals + the enqueued steps);
           beside each step the bytes it moves and the squared distances it evaluates (counted on the host from the grid the
           device built); the same step by torch ops on the device (chunked cdist + argmin, float sums) for comparison.
           HIP-event times.
  host     the route a user has today, for comparison only: download + scipy.spatial.cKDTree + numpy, one step, host clock.
  detect   one GraspDetector.detect of the two views with and without ``register``, alternated; "without" is the baseline.
Warm-up first, then the median of repeated runs with their min / max.

    python scripts/bench_icp.py [--out profiles/icp_register.txt]
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

DEV = "cuda:0"
STEPS = (("kernels", 420), ("host", 300), ("detect", 420))     # (name, time limit in seconds)
WIDTH, HEIGHT = 640, 480
STRIDES = (1, 4, 3)
DETECT_STRIDE = 3                                               # does not divide the width: IcpParams' docstring
MAX_DIST, ITERATIONS = 0.02, 30
FUSE = {"voxel": 0.005, "max_voxels": 1 << 20}


def scene(width=WIDTH, height=HEIGHT):
    """-> (MultiView with the second pose off, the clouds on the device, the given poses, the true poses)."""
    from regnet_for_3d_grasping_amd import depth_frame, fusion
    from tests import fuse_reference, icp_reference
    frames, truth = fuse_reference.two_view_scene(width, height)
    given = [truth[0], icp_reference.perturbation(0.5, 4.0) @ truth[1]]
    mv = fusion.MultiView([depth_frame.DepthFrame(**kw) for kw in frames], given)
    clouds = [depth_frame.to_cloud(frame, device=DEV) for frame in mv.frames]
    return mv, clouds, given, truth


def search_counts(target, source_p, stride):
    """Squared distances one step evaluates: per visited source point the target rows in the cells overlapping its ball, counted
    on the host from the cell edge the device chose -> (distance tests, cell edge, cells)."""
    import numpy as np
    hdr = target.ws[:64].cpu().numpy()
    lo, h = hdr.view(np.float32)[:3].astype(np.float64), float(hdr.view(np.float32)[3])
    dim = hdr.view(np.int32)[5:8].astype(np.int64)
    cell = np.clip(np.floor((target.xyz.cpu().numpy().astype(np.float64) - lo) / h).astype(np.int64), 0, dim - 1)
    count = np.zeros(tuple(dim + 2), dtype=np.int64)                       # one empty cell of margin on every side
    np.add.at(count, tuple((cell + 1).T), 1)
    box = sum(count[1 + dx:dim[0] + 1 + dx, 1 + dy:dim[1] + 1 + dy, 1 + dz:dim[2] + 1 + dz]
              for dx in (-1, 0, 1) for dy in (-1, 0, 1) for dz in (-1, 0, 1))              # rows in the 27 cells around a cell
    p = source_p[::stride]
    p = p[np.isfinite(p).all(axis=1)]
    pc = np.clip(np.floor((p.astype(np.float64) - lo) / h).astype(np.int64), 0, dim - 1)
    return int(box[tuple(pc.T)].sum()), h, int(dim.prod())


def torch_step(source, target_xyz, normals, pose, max_dist, stride, chunk=4096):
    """The same step by torch ops on the device: chunked cdist + argmin, the normal equations by float64 matrix products."""
    import torch
    src = source[::stride]
    src = src[torch.isfinite(src).all(dim=1)]
    p = src @ pose[:3, :3].t() + pose[:3, 3]
    best_d, best_j = [], []
    for k in range(0, p.shape[0], chunk):
        d = torch.cdist(p[k:k + chunk], target_xyz)
        m = d.min(dim=1)
        best_d.append(m.values)
        best_j.append(m.indices)
    d, j = torch.cat(best_d), torch.cat(best_j)
    keep = d <= max_dist
    p, q, n = p[keep].double(), target_xyz[j[keep]].double(), normals[j[keep]].double()
    r = ((p - q) * n).sum(dim=1)
    a = torch.cat((torch.cross(p, n, dim=1), n), dim=1)
    return a.t() @ a, a.t() @ r


def step_kernels(lines):
    import numpy as np
    import torch
    from regnet_for_3d_grasping_amd import fusion, registration
    from tests import icp_reference
    _, clouds, given, truth = scene()
    source = clouds[1][0]
    target_cloud = fusion.transform_cloud(clouds[0][0], given[0])
    base = {"max_dist": MAX_DIST, "iterations": ITERATIONS}
    target = registration.prepare_target(target_cloud, base, target_camera=tuple(given[0][:3, 3]))
    n_t, n_s = target.n, int(source.shape[0])
    prep_normals = timed(lambda: registration.prepare_target(target_cloud, base, target_camera=tuple(given[0][:3, 3])), 2, 10)
    prep_grid = timed(lambda: registration.prepare_target(target_cloud, base, target_normals=target.normals), 2, 10)
    lines.append("target: %d finite rows of %d; prepare_target with the normals given %s;  with the normals estimated %s" % (
        n_t, int(target_cloud.shape[0]), fmt(prep_grid), fmt(prep_normals)))
    source_p = icp_reference.transform(source.cpu().numpy(), given[1])
    pose32 = torch.from_numpy(given[1]).to(DEV).float()
    for stride in STRIDES:
        params = dict(base, stride=stride)
        fresh = torch.from_numpy(registration.initial_state(given[1], params)).to(DEV)
        state = fresh.clone()

        def one():
            state.copy_(fresh)                                             # (a 1152-byte copy: the step must find RUNNING)
            registration.step(source, target, state, params)
        copy = timed(lambda: state.copy_(fresh), 5, 50)
        t_step = timed(one, 5, 50)
        rows = -(-n_s // stride)
        tests, h, cells = search_counts(target, source_p, stride)
        pairs = int(registration.decode_state(state.cpu().numpy())["pairs"])
        moved = rows * 12 + tests * 16 + pairs * 12 + (-(-rows // 256)) * 2 * 232
        lines.append("step  stride %d: %d visited rows, %d pairs  %s  (of it the state copy %.3f ms);  %d distance tests = %.1f per "
                     "visited row over a grid of %d cells, edge %.4f m (requested %.4f);  %.1f MB loaded by the lanes, a count and not "
                     "measured traffic (12 B per row, 16 B per test, 12 B of normal per pair, the partial sums)" % (
                         stride, rows, pairs, fmt(t_step), statistics.median(copy), tests, tests / max(rows, 1), cells, h, MAX_DIST,
                         moved / 1e6))
        whole = timed(lambda: registration.icp(source, target_cloud, given[1], params, target_camera=tuple(given[0][:3, 3])), 2, 10)
        enq = timed(lambda: registration.icp(source, target, given[1], params), 2, 10)
        reg = registration.icp(source, target, given[1], params)
        lines.append("icp   stride %d: whole registration (prepare, normals, %d steps enqueued) %s;  on the prepared target %s;  "
                     "%s after %d iterations, rms %.3g -> %.3g m, pose error %.3g -> %.3g" % (
                         stride, ITERATIONS, fmt(whole), fmt(enq), registration.STATUS_NAMES[reg.status], reg.iterations,
                         reg.rms_first, reg.rms_last, icp_reference.pose_distance(given[1], truth[1]),
                         icp_reference.pose_distance(reg.pose(), truth[1])))
        t_torch = timed(lambda: torch_step(source, target.xyz, target.normals, pose32, MAX_DIST, stride), 2, 10)
        lines.append("torch stride %d: the same step by torch ops (chunked cdist + argmin, %d x %d distances)  %s" % (
            stride, rows, n_t, fmt(t_torch)))
    return True


def step_host(lines):
    import numpy as np
    import torch
    from scipy.spatial import cKDTree
    from regnet_for_3d_grasping_amd import fusion, registration
    _, clouds, given, _ = scene()
    source = clouds[1][0]
    target = registration.prepare_target(fusion.transform_cloud(clouds[0][0], given[0]), {"max_dist": MAX_DIST},
                                         target_camera=tuple(given[0][:3, 3]))
    torch.cuda.synchronize()
    parts = []
    for stride in STRIDES:
        def host():
            t0 = time.perf_counter()
            tgt, nrm = target.xyz.cpu().numpy().astype(np.float64), target.normals.cpu().numpy().astype(np.float64)
            src = source.cpu().numpy().astype(np.float64)[::stride]
            src = src[np.isfinite(src).all(axis=1)]
            p = src @ given[1][:3, :3].T + given[1][:3, 3]
            d, j = cKDTree(tgt).query(p, distance_upper_bound=MAX_DIST)
            keep = np.isfinite(d)
            p, q, n = p[keep], tgt[j[keep]], nrm[j[keep]]
            r = ((p - q) * n).sum(axis=1)
            a = np.concatenate((np.cross(p, n), n), axis=1)
            np.linalg.solve(a.T @ a, -(a.T @ r))
            return (time.perf_counter() - t0) * 1e3
        host()
        parts.append("stride %d  %s" % (stride, fmt(sorted(host() for _ in range(5)))))
    lines.append("host route, one step (download + cKDTree build and query + numpy normal equations, host clock, comparison only)  "
                 + ";  ".join(parts))
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
    plain = detect.GraspDetector(score_net, region_net, fuse=FUSE)
    refining = detect.GraspDetector(score_net, region_net, fuse=FUSE, register={"max_dist": MAX_DIST, "iterations": ITERATIONS,
                                                                               "stride": DETECT_STRIDE})
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
        once(plain)
        once(refining)
    times = {"plain": [], "register": []}
    for _ in range(10):                              # alternated: both see the same neighbours on the machine
        ms, base = once(plain)
        times["plain"].append(ms)
        ms, out = once(refining)
        times["register"].append(ms)
    a, b = sorted(times["plain"]), sorted(times["register"])
    diff = statistics.median(b) - statistics.median(a)
    lines.append("GraspDetector.detect, two 640 x 480 views merged at %g m (%d -> %d merged points; register: stride %d, status %d "
                 "after %d iterations)  without register (baseline) %s;  with register %s;  difference of the medians %+.3f ms = "
                 "%+.2f%% of the frame time" % (FUSE["voxel"], int(base["fuse_num"][0]), int(out["fuse_num"][0]), DETECT_STRIDE,
                                                int(out["fuse_register"][1, 0]), int(out["fuse_register"][1, 1]), fmt(a), fmt(b),
                                                diff, 100.0 * diff / statistics.median(a)))
    return True


def run_step(name, path):
    import torch
    assert torch.cuda.is_available(), "this measurement needs the MI355X"
    lines = []
    ok = {"kernels": step_kernels, "host": step_host, "detect": step_detect}[name](lines)
    with open(path, "w") as f:
        json.dump(lines, f)
    return 0 if ok else 1


def main():
    parser = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    parser.add_argument("--out", default=os.path.join(REPO, "profiles", "icp_register.txt"))
    parser.add_argument("--step", choices=[name for name, _ in STEPS], help="(internal) run one step in this process")
    parser.add_argument("--step-out", help="(internal) where the step leaves its lines")
    args = parser.parse_args()
    if args.step:
        sys.exit(run_step(args.step, args.step_out))
    import torch
    lines = ["pose refinement on the device (scripts/bench_icp.py): %s, torch %s; two %d x %d views, max_dist %g m, %d steps "
             "enqueued; median of HIP-event times unless a host clock is named" % (
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
