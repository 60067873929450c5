"""What object segmentation costs on the MI355X (segment.py, csrc/cluster.hip) -> profiles/cluster_objects.txt.

Four lines of results in three steps, each a fresh child process under its own time limit; the driver stops at the first one
that fails:
  kernels  cluster_points at N = 25 600 and N = 307 200 (one aligned 640 x 480 frame) of a seeded table scene: the whole call and
           the share of it that is its kernels (both stages launched on preallocated buffers with the ranking already in place);
           assign_grasps at Q = 4000 against both N.  HIP-event times.
  host     the route a user has today, for comparison only: download + cKDTree.query_pairs + connected_components, host clock.
  detect   one GraspDetector.detect of the synthetic camera frame with and without ``segment``, alternated; "without" is the
           baseline, the difference is reported in ms and as a share of the frame time.
Warm-up first, then the median of repeated runs with their min / max.

    python scripts/bench_cluster.py [--out profiles/cluster_objects.txt]
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
from bench_grasp_nms import BOUNDS, camera_frame, fmt, timed  # noqa: E402

DEV = "cuda:0"
STEPS = (("kernels", 300), ("host", 300), ("detect", 420))     # (name, time limit in seconds)
SIZES = (25600, 307200)
TOLERANCE, MIN_POINTS, MAX_OBJECTS = 0.01, 50, 64


def table_scene(n, seed):
    """(n,3) float32 in the table frame: a 1.1 x 0.9 m table top at z = 0.75 with 1.5 mm noise and eight boxes of 6..16 cm on it,
    rows in a seeded order."""
    import numpy as np
    rng = np.random.RandomState(seed)
    x, y = rng.uniform(-0.6, 0.5, n), rng.uniform(0.0, 0.9, n)
    z = np.full(n, 0.75)
    for k in range(8):
        cx, cy = -0.45 + 0.25 * (k % 4), 0.25 + 0.4 * (k // 4)
        half, tall = 0.03 + 0.007 * k, 0.05 + 0.02 * k
        z[(np.abs(x - cx) < half) & (np.abs(y - cy) < half)] = 0.75 + tall
    z += rng.normal(0.0, 0.0015, n)
    return np.ascontiguousarray(np.stack([x, y, z], axis=1).astype(np.float32))


def step_kernels(lines):
    import numpy as np
    import torch
    from regnet_for_3d_grasping_amd import _lib, segment
    rng = np.random.RandomState(7)
    for n in SIZES:
        xyz = torch.from_numpy(table_scene(n, n)).to(DEV)
        mask = segment.above_table_mask(xyz, 0.75, 0.01)
        seg = segment.cluster_points(xyz, mask, TOLERANCE, MIN_POINTS, MAX_OBJECTS)
        count, kept, size, _, _ = seg.objects()
        whole = timed(lambda: segment.cluster_points(xyz, mask, TOLERANCE, MIN_POINTS, MAX_OBJECTS), 5, 30)
        # the kernels alone: both stages on preallocated buffers, the ranking (one torch.sort) already in place
        m8 = mask.to(torch.uint8)
        ws = torch.empty((segment.workspace_bytes(n, MAX_OBJECTS),), dtype=torch.uint8, device=DEV)
        i32 = lambda *shape: torch.empty(shape, dtype=torch.int32, device=DEV)
        root, key, label, num, osize, first = i32(n), i32(n), i32(n), i32(2), i32(MAX_OBJECTS), i32(MAX_OBJECTS)
        bbox = torch.empty((MAX_OBJECTS, 6), dtype=torch.float32, device=DEV)

        def launch(stages, order_ptr):
            _lib.call("regnet_cluster_points_f32", xyz, xyz.data_ptr(), m8.data_ptr(), n, TOLERANCE, MIN_POINTS, MAX_OBJECTS,
                      root.data_ptr(), key.data_ptr(), order_ptr, label.data_ptr(), num.data_ptr(), osize.data_ptr(),
                      first.data_ptr(), bbox.data_ptr(), ws.data_ptr(), stages)
        launch(1, 0)
        order = torch.sort(key, descending=True, stable=True).indices
        alone = timed(lambda: launch(3, order.data_ptr()), 5, 30)
        assert torch.equal(label, seg.label)
        share = 100.0 * statistics.median(alone) / statistics.median(whole)
        lines.append("cluster_points  N = %6d (%d above the table, %d objects of %d kept, largest %d)  whole call %s;  "
                     "kernels alone %s = %.0f%% of it" % (n, int(mask.sum()), count, kept, size[0] if count else 0, fmt(whole),
                                                          fmt(alone), share))
        centres = xyz[torch.from_numpy(rng.randint(0, n, 4000)).to(DEV)] + 0.01 * torch.randn((4000, 3), device=DEV)
        grasp = torch.zeros((4000, 8), device=DEV)
        grasp[:, :3] = centres
        assign = timed(lambda: segment.assign_grasps(grasp, xyz, seg.label, 0.03), 5, 30)
        obj, _ = segment.assign_grasps(grasp, xyz, seg.label, 0.03)
        lines.append("assign_grasps   Q = 4000, N = %6d (%d on an object)  %s" % (n, int((obj >= 0).sum()), fmt(assign)))
    return True


def step_host(lines):
    import numpy as np
    import torch
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    from scipy.spatial import cKDTree
    parts = []
    for n in SIZES:
        xyz = torch.from_numpy(table_scene(n, n)).to(DEV)
        torch.cuda.synchronize()

        def host():
            t0 = time.perf_counter()
            pts = xyz.cpu().numpy().astype(np.float64)
            pts = pts[pts[:, 2] > 0.76]
            pairs = cKDTree(pts).query_pairs(TOLERANCE, output_type="ndarray")
            graph = coo_matrix((np.ones(len(pairs), dtype=np.int8), (pairs[:, 0], pairs[:, 1])), shape=(len(pts), len(pts)))
            connected_components(graph, directed=False)
            return (time.perf_counter() - t0) * 1e3
        host()
        parts.append("N = %d  %s" % (n, fmt(sorted(host() for _ in range(5)))))
    lines.append("host route (download + cKDTree.query_pairs + connected_components, host clock, comparison only)  " + ";  ".join(parts))
    return True


def step_detect(lines):
    import contextlib
    import io
    import numpy as np
    import torch
    from regnet_for_3d_grasping_amd import detect, pipeline, synthetic
    from regnet_for_3d_grasping_amd.get_regiondataset import get_grasp_allobj
    frame = camera_frame()
    score_net, region_net = pipeline.build_models(DEV)
    score_net.eval()
    region_net.eval()
    plain = detect.GraspDetector(score_net, region_net, bounds=BOUNDS)
    segmenting = detect.GraspDetector(score_net, region_net, bounds=BOUNDS, segment={})
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
        once(segmenting)
    times = {"plain": [], "segment": []}
    for _ in range(15):                              # alternated: both see the same neighbours on the machine
        times["plain"].append(once(plain)[0])
        ms, out = once(segmenting)
        times["segment"].append(ms)
    a, b = sorted(times["plain"]), sorted(times["segment"])
    diff = statistics.median(b) - statistics.median(a)
    lines.append("GraspDetector.detect, synthetic camera frame (%d points, %d objects, %d of %d grasps on one)  without segment "
                 "(baseline) %s;  with segment %s;  difference of the medians %+.3f ms = %+.2f%% of the frame time" % (
                     len(out["points"]), len(out["object_size"]), int((out["grasp_object"] >= 0).sum()),
                     len(out["grasp_object"]), fmt(a), fmt(b), diff, 100.0 * diff / statistics.median(a)))
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
    parser.add_argument("--out", default=os.path.join(REPO, "profiles", "cluster_objects.txt"))
    parser.add_argument("--step", choices=[name for name, _ in STEPS], help="(internal) run one step in this process")
    parser.add_argument("--step-out", help="(internal) where the step leaves its lines")
    args = parser.parse_args()
    if args.step:
        sys.exit(run_step(args.step, args.step_out))
    import torch
    lines = ["object segmentation on the device (scripts/bench_cluster.py): %s, torch %s; tolerance %g m, min_points %d, "
             "max_objects %d; median of HIP-event times unless a host clock is named" % (
                 torch.cuda.get_device_name(0) if torch.cuda.is_available() else "no GPU", torch.__version__, TOLERANCE,
                 MIN_POINTS, MAX_OBJECTS), ""]
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
