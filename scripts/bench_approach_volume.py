"""What the approach analysis against the TSDF volume costs on the MI355X (approach.analyse_volume, csrc/approach_volume.hip)
-> profiles/approach_volume.txt.

Two steps, each a fresh child process under its own time limit; the driver stops at the first one that fails:
  kernels  the rendered two-view volume of scripts/bench_tsdf.py (320^3 voxels of 2 mm) and B = 16 and B = 4000 grasps centred on
           seeded rows of its surface: the kernel alone, ``analyse_volume`` without and with the contact pass on the surface,
           ``approach.analyse`` on the extracted surface cloud beside it, and the same classification written in torch ops (a
           (B, samples) gather).  The lookups of a call (B x samples, one W and at most one D of 4 bytes each) are reported as a
           count, not as traffic: neighbouring samples share cache lines and nobody has measured what reaches HBM.
  detect   one GraspDetector.detect of the two-view MultiView with ``approach`` in volume space against cloud space, alternated.
Times are HIP events (kernels step) or a host clock around a call that ends in a download (detect step): warm-up first, then
the median of repeated runs with their min / max.  No time is gated.

    python scripts/bench_approach_volume.py [--out profiles/approach_volume.txt]
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
STEPS = (("kernels", 420), ("detect", 420))     # (name, time limit in seconds)
DEPTH, WIDTH = 0.06, 0.08
STANDOFF = 0.10


def torch_formulation(vol, L, box, standoff, step, samples):
    """The same counts and values by torch ops on the device: the lattice as a (samples) list, a (B, samples) gather of W and D."""
    import torch
    x_lo, x_hi, _, ht, hw, hs, back_x = box
    p = vol.params
    n_x, n_y, n_z = samples
    dev = L.device
    xs = x_lo - standoff
    i, j, k = torch.meshgrid(torch.arange(n_x, device=dev), torch.arange(n_y, device=dev), torch.arange(n_z, device=dev), indexing="ij")
    x = (xs + (i.float() + 0.5) * step).reshape(-1)
    y = ((j.float() + 0.5) * step - hw).reshape(-1)
    z = ((k.float() + 0.5) * step - ht).reshape(-1)
    section = (z < ht) & (z > -ht) & (y < hw) & (y > -hw)
    inner = section & (y < hs) & (y > -hs)
    close = (x > x_lo) & (x < x_hi)
    region = inner & close
    hand = (section & close & (x < back_x)).int() + (section & close & ((y > hs) | (y < -hs))).int()
    blocker = section & (x < torch.where(inner, back_x, x_hi)) & (x > xs)
    member = hand + blocker.int()
    retreat = (x_lo - x).clamp(min=0.0)
    l = L.view(-1, 3, 4)
    local = torch.stack((x, y, z), 0)
    w = l[:, :, :3] @ local + l[:, :, 3:4]                                     # (B, 3, samples)
    origin = torch.tensor(vol.origin, device=dev).view(1, 3, 1)
    c = torch.floor((w - origin) / p.voxel)
    dims = torch.tensor(p.dims, device=dev, dtype=torch.float32).view(1, 3, 1)
    inside = ((c >= 0) & (c < dims)).all(1)
    ci = torch.where(inside.unsqueeze(1), c, torch.zeros_like(c)).long()
    v = (ci[:, 2] * p.dims[1] + ci[:, 1]) * p.dims[0] + ci[:, 0]
    W, D = vol.W[v], vol.D[v]
    known = inside & (W >= p.min_weight) & ~torch.isnan(D)
    solid = known & (D < 0.0)
    unseen = ~known
    inf = float("inf")
    counts = torch.stack(((solid & region).sum(1), (unseen & region).sum(1), (solid * hand).sum(1), (unseen * hand).sum(1),
                          (solid & blocker).sum(1), (unseen & blocker).sum(1), member.sum().expand(L.shape[0]),
                          (~inside * member).sum(1)), 1)
    values = torch.stack((torch.where(solid & region, y, inf).amin(1), torch.where(solid & region, y, -inf).amax(1),
                          torch.where(solid & blocker, retreat, inf).amin(1).clamp(max=standoff),
                          torch.where((solid | unseen) & blocker, retreat, inf).amin(1).clamp(max=standoff)), 1)
    return counts, values


def step_kernels(lines):
    import numpy as np
    import torch
    from regnet_for_3d_grasping_amd import _lib, approach, approach_volume, eval_collision, tsdf
    mv, views = scene()
    params = tsdf.TsdfParams(origin=ORIGIN)
    vol = tsdf.Volume(params, DEV)
    for v in (0, 1):
        vol.integrate(views[v], mv.poses[v])
    surface = vol.extract()
    k, _, observed = surface.check()
    cloud = surface.xyz[:k].contiguous()
    lines.append("volume %d x %d x %d voxels of %g m, two views integrated: %d observed voxels, %d surface rows (max_points %d)" % (
        params.dims + (params.voxel, observed, k, params.max_points)))
    rng = np.random.default_rng(11)
    host_cloud = cloud.cpu().numpy()
    for B in (16, 4000):
        grasp = np.zeros((B, 8), dtype=np.float32)
        grasp[:, :3] = host_cloud[rng.integers(0, k, B)] + rng.normal(0.0, 0.01, (B, 3))
        grasp[:, 3:6] = rng.standard_normal((B, 3))
        grasp[:, 6] = rng.uniform(-3.0, 3.0, B)
        grasp = torch.from_numpy(grasp).to(DEV)
        res = approach.analyse_volume(vol, grasp, DEPTH, WIDTH, {"standoff": STANDOFF})
        box, _ = eval_collision._box_args(DEPTH, WIDTH, B, grasp.device)
        samples = res.samples
        n_samples = samples[0] * samples[1] * samples[2]
        counts, values = torch.empty_like(res.counts), torch.empty_like(res.values)

        def kernel():
            _lib.call("regnet_grasp_approach_volume_f32", vol.data, vol.data.data_ptr(), *params.dims, vol.origin.ctypes.data,
                      float(params.voxel), float(params.trunc), int(params.min_weight), 0.0, res.L.data_ptr(), B, *box, STANDOFF,
                      float(params.voxel), DEPTH, counts.data_ptr(), values.data_ptr())

        t_kernel = timed(kernel, 3, 20)
        t_plain = timed(lambda: approach.analyse_volume(vol, grasp, DEPTH, WIDTH, {"standoff": STANDOFF}), 3, 20)
        t_contact = timed(lambda: approach.analyse_volume(vol, grasp, DEPTH, WIDTH, {"standoff": STANDOFF, "friction_deg": 30.0},
                                                          surface=surface), 3, 10)
        t_cloud = timed(lambda: approach.analyse(cloud, grasp, DEPTH, WIDTH, {"standoff": STANDOFF}), 3, 20)
        chunk = max(1, (1 << 24) // n_samples)

        def torch_ops():
            return [torch_formulation(vol, res.L[s:s + chunk], box, STANDOFF, float(np.float32(params.voxel)), samples)
                    for s in range(0, B, chunk)]

        t_torch = timed(torch_ops, 1, 3)
        want = torch.cat([c for c, _ in torch_ops()])
        differ = int((want.to(torch.int32) != res.counts).any(1).sum())
        med = statistics.median
        c = res.counts
        lines.append("B = %d grasps, step %g m: %d x %d x %d = %d samples per grasp, %d lookups per call (8 B each at most; a count, "
                     "not traffic)" % ((B, params.voxel) + samples + (n_samples, B * n_samples)))
        lines.append("    %d grasps with the whole standoff free of seen surfaces, %d also of unseen space; mean unseen share %.3f; "
                     "%d with a solid sample in the hand" % (int((res.clearance_seen >= STANDOFF).sum()), int((res.clearance_safe >= STANDOFF).sum()),
                                                             float(res.unseen_share.mean()), int((c[:, 2] > 0).sum())))
        lines.append("    the kernel alone                          %s" % fmt(t_kernel))
        lines.append("    analyse_volume                            %s" % fmt(t_plain))
        lines.append("    analyse_volume, contact on the surface    %s   (regnet_grasp_approach_f32 over all %d rows of the surface)" % (
            fmt(t_contact), params.max_points))
        lines.append("    approach.analyse on the %7d-row cloud  %s   -> the volume kernel costs %.2fx of it" % (
            k, fmt(t_cloud), med(t_kernel) / med(t_cloud)))
        lines.append("    torch ops, (B, samples) gather, chunked   %s   -> the kernel is %.1fx faster" % (fmt(t_torch), med(t_torch) / med(t_kernel)))
        lines.append("    (grasps whose counts differ from the torch formulation's, whose matmul rounds otherwise: %d of %d)" % (differ, B))
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
    detectors = {"cloud": detect.GraspDetector(score_net, region_net, volume={"origin": ORIGIN}, approach={"space": "cloud"}),
                 "volume": detect.GraspDetector(score_net, region_net, volume={"origin": ORIGIN}, approach={"space": "volume"})}
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
    a, b = sorted(times["cloud"]), sorted(times["volume"])
    diff = statistics.median(b) - statistics.median(a)
    lines.append("GraspDetector.detect of two 640 x 480 views through the volume, host clock, %d grasps of grasp_stage3 analysed:" % len(out["grasp_stage3"]))
    lines.append("    approach in cloud space    %s" % fmt(a))
    lines.append("    approach in volume space   %s" % fmt(b))
    lines.append("    difference of the medians  %+9.3f ms = %+.2f%% of the frame time" % (diff, 100.0 * diff / statistics.median(a)))
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
    parser.add_argument("--out", default=os.path.join(REPO, "profiles", "approach_volume.txt"))
    parser.add_argument("--step", choices=[name for name, _ in STEPS], help="(internal) run one step in this process")
    parser.add_argument("--step-out", help="(internal) where the step leaves its lines")
    args = parser.parse_args()
    if args.step:
        sys.exit(run_step(args.step, args.step_out))
    import torch
    lines = ["approach analysis against the TSDF volume (scripts/bench_approach_volume.py): %s, torch %s" % (
        torch.cuda.get_device_name(0) if torch.cuda.is_available() else "no GPU", torch.__version__),
        "gripper 8 cm x 6 cm, standoff %.2f m, step = the 2 mm voxel; grasps seeded on the surface of scripts/bench_tsdf.py's two-view "
        "volume; median of HIP-event times unless a host clock is named" % STANDOFF, ""]
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
