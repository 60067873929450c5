"""What turning a depth frame into a cloud costs on the MI355X (depth_frame.to_cloud, csrc/depth.hip) -> profiles/depth_frame.txt.

Two steps, each a fresh child process under its own time limit; the driver stops at the first one that fails:
  kernels  to_cloud on the seeded synthetic depth frame (tests/depth_reference.synthetic_depth_frame) at 640 x 480 and
           1280 x 720, aligned and registered colour, images resident on the device, into preallocated outputs: the whole call
           against its byte bound (bytes moved over 8 TB/s of HBM); against (a) the same result written in torch ops on the
           device and (b) today's host route: numpy deprojection to float64 and the upload of both (M,3) float64 arrays.
           Also the whole call from HOST images (upload of 2 + 3 bytes per pixel included), which is what (b) competes with.
  detect   one GraspDetector.detect of the 640 x 480 depth frame against detect of the same cloud handed over as host
           (xyz, rgb) float64 arrays, alternated.
Times are HIP events (device work) or a host clock around work that ends in a synchronise (anything with a host part): warm-up
first, then the median of repeated runs with their min / max.

    python scripts/bench_depth_frame.py [--out profiles/depth_frame.txt]
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
HBM_BYTES_PER_S = 8.0e12
FILTER = {"edge_threshold": 0.02, "min_neighbours": 2}


def timed(fn, warmup, repeats):
    """-> sorted HIP-event times of ``fn()`` in milliseconds."""
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


def host_timed(fn, warmup, repeats):
    """-> sorted host-clock times of ``fn()`` followed by a device synchronise, in milliseconds."""
    import torch
    for _ in range(warmup):
        fn()
    times = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
    return sorted(times)


def fmt(times):
    return "%9.4f ms  (min %.4f, max %.4f, %d runs)" % (statistics.median(times), times[0], times[-1], len(times))


def torch_formulation(depth, color, consts, W, H, t, k, registered=None):
    """(a): the contract in torch ops on the device (deprojection, the 8-neighbour filter through padded shifts, the table
    lookup; registered: projection, scatter-amin z-buffer at splat 0, gather) -> (xyz, rgb)."""
    import torch
    import torch.nn.functional as F
    rfx, rfy, cx, cy, s = (float(v) for v in consts[:5])
    z = depth.to(torch.float32) * s
    valid = depth != 0
    zp = F.pad(z[None, None], (1, 1, 1, 1))[0, 0]
    vp = F.pad(valid[None, None], (1, 1, 1, 1))[0, 0]
    jump = torch.zeros_like(valid)
    count = torch.zeros((H, W), dtype=torch.int32, device=depth.device)
    for dy in range(3):
        for dx in range(3):
            if dy == 1 and dx == 1:
                continue
            zq, vq = zp[dy:dy + H, dx:dx + W], vp[dy:dy + H, dx:dx + W]
            jump |= vq & ((z - zq).abs() > t * torch.minimum(z, zq))
            count += vq
    keep = valid & ~jump & (count >= k)
    u = torch.arange(W, dtype=torch.float32, device=depth.device)[None, :]
    v = torch.arange(H, dtype=torch.float32, device=depth.device)[:, None]
    pts = torch.stack([((u - cx) * z) * rfx, ((v - cy) * z) * rfy, z], dim=-1)
    lut = torch.arange(256, dtype=torch.float64, device=depth.device).div(255.0).to(torch.float32)
    if registered is None:
        rgb = lut[color.long()]
    else:
        R, tr, (fxc, fyc, cxc, cyc), Wc, Hc, margin = registered
        q = pts @ R.t() + tr
        ok = keep & (q[..., 2] > 0)
        fu = torch.floor(q[..., 0] / q[..., 2] * fxc + cxc + 0.5)
        fv = torch.floor(q[..., 1] / q[..., 2] * fyc + cyc + 0.5)
        ok &= (fu >= 0) & (fu < Wc) & (fv >= 0) & (fv < Hc)
        pix = torch.where(ok, fv * Wc + fu, torch.zeros_like(fu)).long().reshape(-1)
        zb = torch.full((Wc * Hc,), float("inf"), device=depth.device)
        zb.scatter_reduce_(0, pix[ok.reshape(-1)], q[..., 2].reshape(-1)[ok.reshape(-1)], reduce="amin")
        keep = ok & (q[..., 2] - zb[pix].reshape(H, W) <= margin)
        rgb = lut[color.reshape(-1, 3)[pix].long()].reshape(H, W, 3)
    nan = torch.full_like(pts, float("nan"))
    return torch.where(keep[..., None], pts, nan).reshape(-1, 3), torch.where(keep[..., None], rgb, torch.zeros_like(rgb)).reshape(-1, 3)


def host_route(frame, device):
    """(b): what a user does today -- deproject on the host in float64, colours / 255 in float64, upload both."""
    import numpy as np
    from regnet_for_3d_grasping_amd._frame_util import to_device
    fx, fy, cx, cy = frame.intrinsics
    H, W = frame.depth.shape
    z = frame.depth.astype(np.float64) * 0.001
    z[frame.depth == 0] = np.nan
    u, v = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    xyz = np.stack([(u - cx) * z / fx, (v - cy) * z / fy, z], axis=-1).reshape(-1, 3)
    rgb = frame.color_aligned.reshape(-1, 3).astype(np.float64) / 255.0
    return to_device(xyz, device), to_device(rgb, device)


def step_kernels(lines):
    import numpy as np
    import torch
    from regnet_for_3d_grasping_amd import depth_frame as df
    from tests import depth_reference as ref
    dev = torch.device(DEV)
    for W, H in ((640, 480), (1280, 720)):
        frame = ref.synthetic_depth_frame(width=W, height=H)
        Hc, Wc = frame.color.shape[:2]
        lines.append("%d x %d depth (uint16), colour %d x %d; filter %s" % (W, H, Wc, Hc, FILTER))
        for mode in ("aligned", "registered"):
            kw = ref.frame_kwargs(frame, registered=mode == "registered", aligned=mode == "aligned")
            host_frame = df.DepthFrame(**kw)
            on_dev = df.DepthFrame(**{key: (torch.from_numpy(v).to(dev) if isinstance(v, np.ndarray) and key != "depth_to_color" else v)
                                      for key, v in kw.items()})
            params = df.DepthParams.coerce(FILTER)
            first = df.to_cloud(on_dev, params, return_status=True)
            ws = torch.empty((max(16, df.workspace_bytes(W, H, Wc, Hc, 2)),), dtype=torch.uint8, device=dev)
            out = tuple(first) + (ws,)
            counts = first[3].cpu().tolist()
            n = W * H
            moved = n * (2 + 25) + (3 * n if mode == "aligned" else 0)
            if mode == "registered":      # the z-buffer's fill and its reads and atomics (9 per kept point at splat 1), status and
                moved += 4 * Wc * Hc + counts[6] * (9 + 1) * 4 + n * (1 + 12) + counts[6] * 3      # xyz read again, the colours
            bound = moved / HBM_BYTES_PER_S * 1e3
            times = timed(lambda: df.to_cloud(on_dev, params, return_status=True, out=out), 10, 200)
            lines.append("  %-10s status histogram %s" % (mode, counts))
            lines.append("    to_cloud, images on the device      %s" % fmt(times))
            lines.append("      byte bound (%.2f MB over 8 TB/s): %.4f ms -> the call runs at %.1f%% of the bound's rate" % (
                moved / 1e6, bound, 100.0 * bound / statistics.median(times)))
            from_host = host_timed(lambda: df.to_cloud(host_frame, params, device=dev), 3, 30)
            lines.append("    to_cloud, images from the host      %s   (host clock, upload included)" % fmt(from_host))
            consts = df.pack_params(host_frame, params, df.MODE_REGISTERED if mode == "registered" else df.MODE_ALIGNED)
            reg = None
            if mode == "registered":
                T = torch.from_numpy(np.asarray(frame.depth_to_color, dtype=np.float32)).to(dev)
                reg = (T[:3, :3].contiguous(), T[:3, 3].contiguous(), frame.color_intrinsics, Wc, Hc, 0.01)
            base = timed(lambda: torch_formulation(on_dev.depth, on_dev.color, consts, W, H, 0.02, 2, reg), 3, 30)
            lines.append("    (a) torch ops on the device         %s   -> to_cloud is %.1fx faster" % (
                fmt(base), statistics.median(base) / statistics.median(times)))
            if mode == "aligned":
                route = host_timed(lambda: host_route(frame, dev), 2, 15)
                lines.append("    (b) numpy float64 + upload (today)  %s   (host clock) -> to_cloud from the host is %.1fx faster" % (
                    fmt(route), statistics.median(route) / statistics.median(from_host)))
        lines.append("")
    return True


def step_detect(lines):
    import numpy as np
    import torch
    from regnet_for_3d_grasping_amd import depth_frame as df
    from regnet_for_3d_grasping_amd import detect, np_random, pipeline, synthetic
    from regnet_for_3d_grasping_amd.get_regiondataset import get_grasp_allobj
    from tests import depth_reference as ref
    frame = ref.synthetic_depth_frame()
    kw = ref.frame_kwargs(frame, registered=True)
    depth_frame = df.DepthFrame(**kw)
    xyz, rgb = ref.to_cloud(**kw, **FILTER)[:2]
    cloud = (xyz.astype(np.float64), rgb.astype(np.float64))          # what a .pcd reader or another library hands over today
    score_net, region_net = pipeline.build_models(DEV)
    score_net.eval()
    region_net.eval()
    detector = detect.GraspDetector(score_net, region_net, depth=FILTER)
    np.random.seed(1234)
    with np_random.deferred(), torch.no_grad():
        pc = detector.ingest(cloud).pc.clone()
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

    def once(source):
        np.random.seed(1234)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = detector.detect(source)
        return (time.perf_counter() - t0) * 1e3, out
    for _ in range(3):
        once(cloud)
        once(depth_frame)
    times = {"cloud": [], "depth": []}
    for _ in range(15):                              # alternated: both see the same neighbours on the machine
        times["cloud"].append(once(cloud)[0])
        ms, out = once(depth_frame)
        times["depth"].append(ms)
    a, b = sorted(times["cloud"]), sorted(times["depth"])
    diff = statistics.median(b) - statistics.median(a)
    lines.append("GraspDetector.detect, 640 x 480, registered colour: %d points kept, %d grasps in grasp_stage3" % (
        len(out["points"]), len(out["grasp_stage3"])))
    lines.append("    the cloud as host (xyz, rgb) float64 (today)   %s" % fmt(a))
    lines.append("    the DepthFrame from the host                   %s" % fmt(b))
    lines.append("    difference of the medians                      %+9.3f ms = %+.2f%% of the frame time" % (
        diff, 100.0 * diff / statistics.median(a)))
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
    parser.add_argument("--out", default=os.path.join(REPO, "profiles", "depth_frame.txt"))
    parser.add_argument("--step", choices=[name for name, _ in STEPS], help="(internal) run one step in this process")
    parser.add_argument("--step-out", help="(internal) where the step leaves its lines")
    args = parser.parse_args()
    if args.step:
        sys.exit(run_step(args.step, args.step_out))
    import torch
    lines = ["depth frames on the device (scripts/bench_depth_frame.py): %s, torch %s" % (
        torch.cuda.get_device_name(0) if torch.cuda.is_available() else "no GPU", torch.__version__),
        "seeded synthetic depth frame (5 % holes, mixed pixels at silhouettes); medians of HIP-event times unless marked", ""]
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
