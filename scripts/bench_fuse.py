"""What multi-view fusion costs on the MI355X (fusion.py, csrc/fuse.hip) -> profiles/fuse_views.txt.

Three steps, each a fresh child process under its own time limit; the driver stops at the first one that fails:
  kernels  voxel_merge of 2 and 4 views of 640 x 480 (tests/fuse_reference.two_view_scene, deprojected by to_cloud) at voxels of
           2 mm and 5 mm: the whole call, and on preallocated buffers its parts -- the table fills + accumulate, finalise, the
           torch.sort, emit -- with the byte bound of the call (computed below) at 8 TB/s; the same result by torch ops on the
           device (torch.unique(return_inverse) + index_add_) for comparison.  HIP-event times.
  host     the route without the kernels, for comparison only: download + np.unique + np.add.at, host clock.
  detect   one GraspDetector.detect of a two-view MultiView against one of the first view's DepthFrame, alternated; the single
           view is the baseline.
Warm-up first, then the median of repeated runs with their min / max.

    python scripts/bench_fuse.py [--out profiles/fuse_views.txt]
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
CASES = ((2, 0.002), (2, 0.005), (4, 0.002), (4, 0.005))       # (views, voxel [m])
MAX_VOXELS = 1 << 20
PEAK_BYTES_PER_S = 8e12


def scene(views):
    """-> (MultiView, [(xyz, rgb)] on the device, poses)."""
    from regnet_for_3d_grasping_amd import depth_frame, fusion
    from tests import fuse_reference as ref
    frames, poses = ref.two_view_scene(WIDTH, HEIGHT, views=views)
    mv = fusion.MultiView([depth_frame.DepthFrame(**kw) for kw in frames], poses)
    clouds = [depth_frame.to_cloud(frame, device=DEV) for frame in mv.frames]
    return mv, clouds, poses


def byte_bound(rows, kept, max_voxels):
    """Bytes one merge cannot avoid moving: the rows read once (24 B), the table cleared (92 B per slot) and scanned by the
    compaction (12 B per slot), the key buffer filled (8 B per voxel of capacity), the kept slots read and ranked (92 + 12 B) and
    the outputs written whole (40 B per voxel of capacity).  The atomics' own traffic and the sort's passes are not in it."""
    from regnet_for_3d_grasping_amd import fusion
    slots = fusion.table_slots(max_voxels)
    return rows * 24 + slots * (92 + 12) + max_voxels * (8 + 40) + kept * (92 + 12)


def torch_merge(clouds, poses, voxel):
    """The same centroids by torch ops on the device (float sums: not reproducible bit for bit) -> (xyz, rgb) of the voxels."""
    import torch
    from regnet_for_3d_grasping_amd import fusion
    pts, cols = [], []
    for (xyz, rgb), pose in zip(clouds, poses):
        r = torch.from_numpy(fusion.pose12(pose)).to(xyz.device).view(3, 4)
        ok = torch.isfinite(xyz).all(dim=1)
        pts.append(xyz[ok] @ r[:, :3].t() + r[:, 3])
        cols.append(rgb[ok])
    pts, cols = torch.cat(pts), torch.cat(cols)
    cell = torch.floor(pts * float(1.0 / voxel)).to(torch.int64) + (1 << 20)
    key = (cell[:, 0] << 42) | (cell[:, 1] << 21) | cell[:, 2]
    uniq, inverse, counts = torch.unique(key, return_inverse=True, return_counts=True)
    sums = torch.zeros((uniq.shape[0], 6), dtype=torch.float32, device=pts.device)
    sums.index_add_(0, inverse, torch.cat((pts, cols), dim=1))
    sums /= counts[:, None].to(torch.float32)
    return sums[:, :3], sums[:, 3:]


def step_kernels(lines):
    import numpy as np
    import torch
    from regnet_for_3d_grasping_amd import _lib, fusion
    for views, voxel in CASES:
        _, clouds, poses = scene(views)
        params = fusion.FuseParams(voxel=voxel, max_voxels=MAX_VOXELS)
        fused = fusion.voxel_merge(clouds, poses, params)
        kept, merged, dropped = fused.check()
        rows = sum(int(xyz.shape[0]) for xyz, _ in clouds)
        whole = timed(lambda: fusion.voxel_merge(clouds, poses, params), 5, 30)
        # the parts, on preallocated buffers
        mv = MAX_VOXELS
        ws = torch.empty((fusion.workspace_bytes(mv),), dtype=torch.uint8, device=DEV)
        keys = torch.empty((mv,), dtype=torch.int64, device=DEV)
        out = (fused.xyz, fused.rgb, fused.count, fused.views, fused.first, fused.num)
        origin = np.zeros(3, dtype=np.float32)
        rows12 = [fusion.pose12(p) for p in poses]

        def accumulate():
            offset = 0
            for v, (xyz, rgb) in enumerate(clouds):
                _lib.call("regnet_fuse_accumulate_f32", ws, xyz.data_ptr(), rgb.data_ptr(), int(xyz.shape[0]), v, offset,
                          rows12[v].ctypes.data, origin.ctypes.data, voxel, mv, 1 if v == 0 else 0, ws.data_ptr())
                offset += int(xyz.shape[0])

        def finalise():
            _lib.call("regnet_fuse_finalise_f32", ws, mv, 1, keys.data_ptr(), ws.data_ptr())
        accumulate()
        finalise()
        order = torch.sort(keys).indices

        def emit():
            _lib.call("regnet_fuse_emit_f32", ws, order.data_ptr(), origin.ctypes.data, voxel, mv, *(t.data_ptr() for t in out),
                      ws.data_ptr())
        t_acc, t_fin = timed(accumulate, 5, 30), timed(finalise, 5, 30)
        t_sort, t_emit = timed(lambda: torch.sort(keys), 5, 30), timed(emit, 5, 30)
        emit()
        assert int(fused.num[0]) == kept
        t_torch = timed(lambda: torch_merge(clouds, poses, voxel), 3, 15)
        bound_ms = byte_bound(rows, kept, mv) / PEAK_BYTES_PER_S * 1e3
        med = statistics.median
        lines.append("voxel_merge  %d views of %d x %d, voxel %g m: %d rows (%d dropped) -> %d points, %.1f rows per voxel" % (
            views, WIDTH, HEIGHT, voxel, rows, dropped, kept, merged / max(kept, 1)))
        lines.append("    whole call          %s;  byte bound %.3f ms (%.1f MB at 8 TB/s): the call is %.1f x the bound" % (
            fmt(whole), bound_ms, byte_bound(rows, kept, mv) / 1e6, med(whole) / bound_ms))
        lines.append("    fills + accumulate  %s" % fmt(t_acc))
        lines.append("    finalise            %s" % fmt(t_fin))
        lines.append("    torch.sort          %s = %.0f%% of the whole call" % (fmt(t_sort), 100.0 * med(t_sort) / med(whole)))
        lines.append("    emit                %s" % fmt(t_emit))
        lines.append("    torch.unique + index_add_ on the device (comparison)  %s = %.1f x voxel_merge" % (
            fmt(t_torch), med(t_torch) / med(whole)))
    return True


def step_host(lines):
    import numpy as np
    import torch
    for views, voxel in ((2, 0.002), (4, 0.005)):
        _, clouds, poses = scene(views)
        torch.cuda.synchronize()

        def host():
            t0 = time.perf_counter()
            pts, cols = [], []
            for (xyz, rgb), pose in zip(clouds, poses):
                p, c = xyz.cpu().numpy(), rgb.cpu().numpy()
                ok = np.isfinite(p).all(axis=1)
                T = np.eye(4) if pose is None else np.asarray(pose)
                pts.append(p[ok].astype(np.float64) @ T[:3, :3].T + T[:3, 3])
                cols.append(c[ok].astype(np.float64))
            pts, cols = np.concatenate(pts), np.concatenate(cols)
            cell = np.floor(pts / voxel).astype(np.int64) + (1 << 20)
            key = (cell[:, 0] << 42) | (cell[:, 1] << 21) | cell[:, 2]
            uniq, inverse, counts = np.unique(key, return_inverse=True, return_counts=True)
            sums = np.zeros((len(uniq), 6))
            np.add.at(sums, inverse, np.concatenate((pts, cols), axis=1))
            sums /= counts[:, None]
            return (time.perf_counter() - t0) * 1e3
        host()
        lines.append("host route, %d views, voxel %g m (download + np.unique + np.add.at, host clock, comparison only)  %s" % (
            views, voxel, fmt(sorted(host() for _ in range(3)))))
    return True


def step_detect(lines):
    import contextlib
    import io
    import numpy as np
    import torch
    from regnet_for_3d_grasping_amd import detect, pipeline, synthetic
    from regnet_for_3d_grasping_amd.get_regiondataset import get_grasp_allobj
    mv, _, _ = scene(2)
    single = mv.frames[0]
    score_net, region_net = pipeline.build_models(DEV)
    score_net.eval()
    region_net.eval()
    detector = detect.GraspDetector(score_net, region_net)
    np.random.seed(1234)
    pc = detector.ingest(mv).pc
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

    def once(frame):
        np.random.seed(1234)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = detector.detect(frame)
        return (time.perf_counter() - t0) * 1e3, out
    for _ in range(3):
        once(single)
        once(mv)
    times = {"single": [], "fused": []}
    for _ in range(15):                              # alternated: both see the same neighbours on the machine
        times["single"].append(once(single)[0])
        ms, out = once(mv)
        times["fused"].append(ms)
    a, b = sorted(times["single"]), sorted(times["fused"])
    diff = statistics.median(b) - statistics.median(a)
    lines.append("GraspDetector.detect, 640 x 480 depth frames, default FuseParams (%d merged points of %d rows, %d in the "
                 "workspace)  one view (baseline) %s;  two views fused %s;  difference of the medians %+.3f ms = %+.2f%% of the "
                 "frame time" % (out["fuse_num"][0], out["fuse_num"][1], len(out["points"]), fmt(a), fmt(b), diff,
                                 100.0 * diff / statistics.median(a)))
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
    parser.add_argument("--out", default=os.path.join(REPO, "profiles", "fuse_views.txt"))
    parser.add_argument("--step", choices=[name for name, _ in STEPS], help="(internal) run one step in this process")
    parser.add_argument("--step-out", help="(internal) where the step leaves its lines")
    args = parser.parse_args()
    if args.step:
        sys.exit(run_step(args.step, args.step_out))
    import torch
    lines = ["multi-view fusion on the device (scripts/bench_fuse.py): %s, torch %s; max_voxels 2^20 (a table of 2^21 slots); "
             "median of HIP-event times unless a host clock is named" % (
                 torch.cuda.get_device_name(0) if torch.cuda.is_available() else "no GPU", torch.__version__), ""]
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
