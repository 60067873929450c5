"""What the TSDF volume costs on the MI355X (tsdf.py, csrc/tsdf.hip) -> profiles/tsdf_volume.txt.

Two steps, each a fresh child process under its own time limit; the driver stops at the first one that fails:
  kernels  the two rendered 640 x 480 views of scripts/bench_fuse.py (tests/fuse_reference.two_view_scene, deprojected by
           to_cloud) and the default volume (320^3 voxels of 2 mm, 655 MB) moved onto the scene: ``integrate`` of each view on
           the volume that holds the other, with its share of the byte bound (2 x 20 B per updated voxel + 20 B per voxel only read, at 8 TB/s);
           ``extract`` whole and its count pass, ``torch.cumsum`` and emit pass apart; ``fuse_volume`` of the two views beside
           ``fuse_frames`` of the same two; and ``integrate`` WITHOUT the workgroup early exit (a twin of csrc/tsdf.hip generated
           by scripts/ablate/tsdf_no_early_exit.patch -- neither the vote nor any barrier is left in its layer loop -- and built
           by this script, never part of the library), both orders of the
           views.  HIP-event times.
  detect   one GraspDetector.detect of the two-view MultiView with ``volume`` against one with ``fuse``, alternated.
Warm-up first, then the median of repeated runs with their min / max.

    python scripts/bench_tsdf.py [--out profiles/tsdf_volume.txt]
"""
import argparse
import ctypes
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

DEV = "cuda:0"
STEPS = (("kernels", 420), ("detect", 420))     # (name, time limit in seconds)
WIDTH, HEIGHT = 640, 480
PEAK_BYTES_PER_S = 8e12
PATCH = os.path.join(REPO, "scripts", "ablate", "tsdf_no_early_exit.patch")
TWIN_DIR = os.path.join(REPO, "scripts", "ablate", "tsdf_twin")
ORIGIN = (-0.32, -0.32, 0.7)        # the default 64 cm cube moved onto this scene's table, 0.85 - 1.1 m from the first camera


def scene():
    """-> (MultiView, per view (xyz, rgb, width, height, Intrinsics) on the device)."""
    from regnet_for_3d_grasping_amd import depth_frame, fusion
    from tests import fuse_reference as ref
    frames, poses = ref.two_view_scene(WIDTH, HEIGHT)
    mv = fusion.MultiView([depth_frame.DepthFrame(**kw) for kw in frames], poses)
    views = [depth_frame.to_cloud(frame, device=DEV) + (WIDTH, HEIGHT, frame.intrinsics) for frame in mv.frames]
    return mv, views


def build_twin():
    """csrc/tsdf.hip with the early exit patched out -> a shared object of that one translation unit (built once)."""
    from regnet_for_3d_grasping_amd.csrc import build
    os.makedirs(TWIN_DIR, exist_ok=True)
    src, so = os.path.join(TWIN_DIR, "tsdf_no_early_exit.hip"), os.path.join(TWIN_DIR, "libtsdf_no_early_exit.so")
    with open(PATCH, "rb") as f:
        patch = f.read()
    original = os.path.join(build.HERE, "tsdf.hip")
    res = subprocess.run(["patch", "-s", "-o", src, original], input=patch, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    if res.returncode != 0:
        raise RuntimeError("%s no longer applies to csrc/tsdf.hip:\n%s" % (PATCH, res.stdout.decode(errors="replace")))
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(PATCH), os.path.getmtime(original)):
        subprocess.check_call([build._hipcc()] + build.COMMON + ["-ffp-contract=off", "-I", build.HERE, "-shared", src, "-o", so])
    return so


def step_kernels(lines):
    import numpy as np
    import torch
    from regnet_for_3d_grasping_amd import _lib, fusion, tsdf
    mv, views = scene()
    params = tsdf.TsdfParams(origin=ORIGIN)
    vol = tsdf.Volume(params, DEV)
    n = vol.D.numel()
    lines.append("volume %d x %d x %d voxels of %g m at %s, trunc %g m: %.0f MB (20 B per voxel)" % (
        params.dims + (params.voxel, ORIGIN, params.trunc, vol.bytes / 1e6)))
    med = statistics.median
    twin = ctypes.CDLL(build_twin())
    fn = twin.regnet_tsdf_integrate_f32
    fn.restype, fn.argtypes = _lib.SIGNATURES["regnet_tsdf_integrate_f32"]
    counts_twin = torch.empty((4,), dtype=torch.int32, device=DEV)

    def integrate_twin(view, pose):
        xyz, rgb, w, h, k = view
        intr = np.asarray(k.astuple(), dtype=np.float32)
        status = fn(vol.data.data_ptr(), *params.dims, vol.origin.ctypes.data, params.voxel, params.trunc, params.max_weight,
                    xyz.data_ptr(), rgb.data_ptr(), w, h, intr.ctypes.data, tsdf.camera_from_common(pose).ctypes.data,
                    counts_twin.data_ptr(), torch.cuda.current_stream().cuda_stream)
        assert status == 0

    for order in ((0, 1), (1, 0)):
        first, second = order
        vol.reset()
        vol.integrate(views[first], mv.poses[first])
        for v in (second, first):                  # every timed call updates the volume that already holds both views' voxels
            counts = vol.integrate(views[v], mv.poses[v]).cpu().numpy()
            updated = int(counts[tsdf.UPDATED])
            bound_ms = 2 * 20 * updated / PEAK_BYTES_PER_S * 1e3
            t = timed(lambda: vol.integrate(views[v], mv.poses[v]), 3, 20)
            t_twin = timed(lambda: integrate_twin(views[v], mv.poses[v]), 3, 20)
            integrate_twin(views[v], mv.poses[v])
            assert np.array_equal(counts_twin.cpu().numpy(), counts)
            lines.append("integrate view %d (order %d,%d): updated %d, not in view %d, no depth %d, behind %d of %d voxels" % (
                (v,) + order + tuple(int(c) for c in counts) + (n,)))
            lines.append("    the call              %s;  byte bound %.4f ms (%.1f MB: 2 x 20 B per updated voxel; no voxel is read "
                         "without being written) at 8 TB/s: the call is %.1f x the bound" % (
                             fmt(t), bound_ms, 2 * 20 * updated / 1e6, med(t) / bound_ms))
            lines.append("    without the early exit  %s = %.2f x the call" % (fmt(t_twin), med(t_twin) / med(t)))
    # extraction of the two-view volume, on preallocated outputs
    vol.reset()
    for v in (0, 1):
        vol.integrate(views[v], mv.poses[v])
    surface = vol.extract()
    k, total, observed = surface.check()
    out = (surface.xyz, surface.rgb, surface.normal, surface.weight, surface.num)
    nx, ny, nz = params.dims
    block_counts = torch.empty((int(_lib.lib.regnet_tsdf_blocks(nx, ny, nz)),), dtype=torch.int32, device=DEV)

    def count():
        _lib.call("regnet_tsdf_count", vol.data, vol.data.data_ptr(), nx, ny, nz, params.min_weight, block_counts.data_ptr(),
                  surface.num.data_ptr())
    count()
    base = torch.cumsum(block_counts, 0, dtype=torch.int32) - block_counts

    def emit():
        _lib.call("regnet_tsdf_emit_f32", vol.data, vol.data.data_ptr(), nx, ny, nz, vol.origin.ctypes.data, params.voxel,
                  params.min_weight, block_counts.data_ptr(), base.data_ptr(), params.max_points, *(t.data_ptr() for t in out))
    t_whole = timed(lambda: vol.extract(out=out), 3, 20)
    t_count, t_emit = timed(count, 3, 20), timed(emit, 3, 20)
    t_sum = timed(lambda: torch.cumsum(block_counts, 0, dtype=torch.int32) - block_counts, 3, 20)
    read_ms = 8 * n / PEAK_BYTES_PER_S * 1e3
    lines.append("extract: %d rows of %d observed voxels (max_points %d)" % (k, observed, params.max_points))
    lines.append("    whole call   %s" % fmt(t_whole))
    lines.append("    count pass   %s;  D and W read once (%.0f MB) at 8 TB/s: %.3f ms, the pass is %.1f x that" % (
        fmt(t_count), 8 * n / 1e6, read_ms, med(t_count) / read_ms))
    lines.append("    torch.cumsum %s  (%d blocks of 256 voxels)" % (fmt(t_sum), block_counts.numel()))
    lines.append("    emit pass    %s  (the predicate again, the rows, and the %d sentinel rows)" % (fmt(t_emit), params.max_points - k))
    t_volume = timed(lambda: tsdf.fuse_volume(mv, None, params, device=DEV, volume=vol), 3, 15)
    t_merge = timed(lambda: fusion.fuse_frames(mv, None, None, device=DEV), 3, 15)
    lines.append("two views, to_cloud included:  fuse_volume (reset, 2 x integrate, extract) %s;  fuse_frames (voxel_merge, 2 mm) %s"
                 ";  ratio %.1f" % (fmt(t_volume), fmt(t_merge), med(t_volume) / med(t_merge)))
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
    merged = detect.GraspDetector(score_net, region_net)
    volume = detect.GraspDetector(score_net, region_net, volume={"origin": ORIGIN})
    np.random.seed(1234)
    pc = merged.ingest(mv).pc
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
        once(merged)
        once(volume)
    times = {"fuse": [], "volume": []}
    for _ in range(15):                              # alternated: both see the same neighbours on the machine
        times["fuse"].append(once(merged)[0])
        ms, out = once(volume)
        times["volume"].append(ms)
    a, b = sorted(times["fuse"]), sorted(times["volume"])
    diff = statistics.median(b) - statistics.median(a)
    lines.append("GraspDetector.detect of two 640 x 480 views, host clock:  fuse (default FuseParams) %s;  volume (default TsdfParams, "
                 "%d surface rows, %d in the workspace) %s;  difference of the medians %+.3f ms = %+.2f%% of the frame time" % (
                     fmt(a), out["tsdf_num"][0], len(out["points"]), fmt(b), diff, 100.0 * diff / statistics.median(a)))
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
    parser.add_argument("--out", default=os.path.join(REPO, "profiles", "tsdf_volume.txt"))
    parser.add_argument("--step", choices=[name for name, _ in STEPS], help="(internal) run one step in this process")
    parser.add_argument("--step-out", help="(internal) where the step leaves its lines")
    args = parser.parse_args()
    if args.step:
        sys.exit(run_step(args.step, args.step_out))
    import torch
    lines = ["TSDF volume on the device (scripts/bench_tsdf.py): %s, torch %s; two rendered 640 x 480 views; median of HIP-event "
             "times unless a host clock is named" % (
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
