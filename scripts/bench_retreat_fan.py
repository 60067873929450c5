"""What the retreat fan costs on the MI355X (approach.retreat_fan; regnet_grasp_retreat_fan_signed_f32 and
regnet_grasp_retreat_pick in csrc/retreat.hip) -> profiles/retreat_fan.txt.

Two steps, each a fresh child process under its own time limit; the driver stops at the first one that fails:
  fan      the rendered two-view volume of scripts/bench_tsdf.py (320^3 voxels of 2 mm), its field signed and capped at 10 cm
           (mode solid).  At B = 16, 256 and 4000 grasps about the surface: the fan kernel with the default fan (R = 5, K = 20)
           and the pick; the signed margin kernel on the same grasps in the same run, the yardstick -- by count the fan does
           R (K + 1) times the hand-sample lookups of one margin call, which also looks up the blockers of its sweep, so the
           measured ratio stands beside the ratio of the lookups counted from both kernels' own counts; and the same profile
           by torch index operations on the device, the alternative a user has today.
  detect   one GraspDetector.detect of the two-view MultiView in volume space with ``--approach-signed --approach-field-cap 0.1``
           against one with ``--approach-retreat`` added, alternated; and, because that frame leaves the synthetic networks no
           grasp to analyse, the detector's approach stage alone on 256 fixed proposals about the surface, with and without.
Times are HIP events (fan step) or a host clock around a call that ends in a download (detect step): warm-up first, then the
median of repeated runs with their min / max.  No time is gated.

    python scripts/bench_retreat_fan.py [--out profiles/retreat_fan.txt]
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
from bench_distance_field import DEPTH, DEV, STANDOFF, WIDTH  # noqa: E402
from bench_outliers import fmt, timed  # noqa: E402
from bench_tsdf import ORIGIN, scene  # noqa: E402

STEPS = (("fan", 420), ("detect", 420))         # (name, time limit in seconds)
SIZES = (16, 256, 4000)


def torch_profile(field, vol, L, dirs, K, ds, box, step, x_extent, outside):
    """The fan's profile (B,R,K+1) by torch index operations on the device: the hand's lattice samples of one x_hi for all grasps,
    moved, transformed and looked up as tensors.  Not bit-pinned (torch may contract the products); it is timed, and compared
    with the kernel only as a share of equal words."""
    import torch
    x_lo, x_hi, _, ht, hw, hs, back_x = box
    p = vol.params
    nx, ny, nz = p.dims
    dev = field.dist2.device

    def axis(lo, hi, start=None):
        n = max(1, int(-(-(hi - lo) // step)))
        a = (torch.arange(n, device=dev, dtype=torch.float32) + 0.5) * step
        return a + lo if start is None else a - start
    x, y, z = torch.meshgrid(axis(x_lo, x_extent), axis(-hw, hw, hw), axis(-ht, ht, ht), indexing="ij")
    x, y, z = x.reshape(-1), y.reshape(-1), z.reshape(-1)
    section = (z < ht) & (z > -ht) & (y < hw) & (y > -hw)
    close = (x > x_lo) & (x < x_hi)
    hand = section & close & ((x < back_x) | (y > hs) | (y < -hs))
    pts = torch.stack([x[hand], y[hand], z[hand]], dim=1)                                   # (S,3)
    t = torch.arange(K + 1, device=dev, dtype=torch.float32) * float(ds)
    moved = pts[None, None, :, :] + t[None, :, None, None] * dirs[:, None, None, :]        # (R,K+1,S,3)
    rows = L.view(-1, 3, 4)
    world = torch.einsum("bij,rksj->brksi", rows[:, :, :3], moved) + rows[:, None, None, None, :, 3]
    origin = torch.from_numpy(vol.origin.copy()).to(dev)
    cell = torch.floor((world - origin) / float(p.voxel))
    dims = torch.tensor([nx, ny, nz], device=dev, dtype=torch.float32)
    inside = ((cell >= 0) & (cell < dims)).all(dim=-1)
    c = cell.clamp(min=0).to(torch.int64)
    index = (torch.clamp(c[..., 2], max=nz - 1) * ny + torch.clamp(c[..., 1], max=ny - 1)) * nx + torch.clamp(c[..., 0], max=nx - 1)
    words = field.dist2[index]
    fill = -1 if outside else (1 << 30)
    return torch.where(inside, words, torch.full_like(words, fill)).amin(dim=3)


def step_fan(lines):
    import numpy as np
    import torch
    from regnet_for_3d_grasping_amd import _lib, approach, eval_collision, retreat, tsdf
    mv, views = scene()
    params = tsdf.TsdfParams(origin=ORIGIN)
    vol = tsdf.Volume(params, DEV)
    for v in (0, 1):
        vol.integrate(views[v], mv.poses[v])
    surface = vol.extract()
    k, _, observed = surface.check()
    nx, ny, nz = params.dims
    lines.append("volume %d x %d x %d voxels of %g m, two views integrated: %d observed voxels, %d surface rows" % (
        params.dims + (params.voxel, observed, k)))
    med = statistics.median
    host_cloud = surface.xyz[:k].cpu().numpy()
    field = vol.distance_field("solid", signed=True, max_distance=0.10)
    fan_params = retreat.RetreatParams()
    R, K = 5, int(fan_params.steps)
    ds = float(fan_params.length) / K
    lines.append("field: mode solid, signed, capped at 0.10 m (%d voxels); fan: R = %d directions, K = %d steps of %g m, tilt %g deg, "
                 "lattice step = the voxel" % (field.cap, R, K, ds, fan_params.tilt_deg))
    for B in SIZES:
        grasp = np.zeros((B, 8), dtype=np.float32)
        grng = np.random.default_rng(11)
        grasp[:, :3] = host_cloud[grng.integers(0, k, B)] + grng.normal(0.0, 0.01, (B, 3))
        grasp[:, 3:6] = grng.standard_normal((B, 3))
        grasp[:, 6] = grng.uniform(-3.0, 3.0, B)
        grasp = torch.from_numpy(grasp).to(DEV)
        fan = approach.retreat_fan(vol, field, grasp, DEPTH, WIDTH, fan_params)
        box, _ = eval_collision._box_args(DEPTH, WIDTH, B, grasp.device)
        margins = torch.empty((B, 2), dtype=torch.int32, device=DEV)
        counts = torch.empty((B, 6), dtype=torch.int32, device=DEV)
        profile, result, best = torch.empty_like(fan.profile), torch.empty_like(fan.result), torch.empty_like(fan.best)
        voxel = float(params.voxel)

        def margin():
            _lib.call("regnet_grasp_margin_volume_signed_f32", field.dist2, field.dist2.data_ptr(), nx, ny, nz,
                      vol.origin.ctypes.data, voxel, 0, fan.L.data_ptr(), B, *box, STANDOFF, voxel, DEPTH, margins.data_ptr(),
                      counts.data_ptr())

        def kernel():
            _lib.call("regnet_grasp_retreat_fan_signed_f32", field.dist2, field.dist2.data_ptr(), nx, ny, nz,
                      vol.origin.ctypes.data, voxel, 0, fan.L.data_ptr(), B, *box, voxel, DEPTH, fan.dirs.data_ptr(), 0, R, K, ds,
                      fan.thresh, profile.data_ptr(), result.data_ptr())

        def pick():
            _lib.call("regnet_grasp_retreat_pick", result, result.data_ptr(), B, R, best.data_ptr())

        t_m, t_f, t_p = timed(margin, 3, 20), timed(kernel, 3, 20), timed(pick, 3, 20)
        assert torch.equal(profile, fan.profile) and torch.equal(best, fan.best)
        c = counts.cpu().numpy().astype(np.int64)
        hand, swept = int(c[:, 0].sum()), int(c[:, 2].sum())
        by_count = R * (K + 1) * hand / float(swept)
        lines.append("B = %4d: regnet_grasp_margin_volume_signed_f32 (yardstick)  %s   %d hand of %d swept samples looked up" % (
            B, fmt(t_m), hand, swept))
        lines.append("          regnet_grasp_retreat_fan_signed_f32              %s   %.1fx of the yardstick; by count of lookups "
                     "R (K + 1) hand / swept = %.1fx" % (fmt(t_f), med(t_f) / med(t_m), by_count))
        lines.append("          regnet_grasp_retreat_pick                        %s" % fmt(t_p))
        lines.append("          %.1f G lookups per second in the fan, %.1f G in the margin kernel (counts over the medians)" % (
            R * (K + 1) * hand / med(t_f) * 1e-6, swept / med(t_m) * 1e-6))
        if B <= 256:                                 # (the torch route holds B R (K + 1) S positions: 4000 grasps do not fit a run)
            args = (field, vol, fan.L, fan.dirs, K, ds, [float(v) if v is not None else None for v in box], voxel, DEPTH, 0)
            got = torch_profile(*args)
            t_t = timed(lambda: torch_profile(*args), 2, 8)
            same = float((got == fan.profile).to(torch.float32).mean())
            lines.append("          the same profile by torch index operations       %s   %.0fx of the fan kernel; %.2f%% of its words "
                         "equal the kernel's (torch's arithmetic is not pinned)" % (fmt(t_t), med(t_t) / med(t_f), 100.0 * same))
        steps = fan.free_steps.cpu().numpy()
        index = fan.index.cpu().numpy()
        lines.append("          free steps of the straight retreat: %d of %d grasps free over all %d steps; the pick leaves straight "
                     "for %d grasps; %d grasps with no free step in any direction" % (
                         int((steps[:, 0] == K).sum()), B, K, int((index != 0).sum()), int((steps.max(axis=1) == 0).sum())))
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
    signed = {"space": "volume", "field": True, "field_signed": True, "field_max_distance": 0.1}
    detectors = {"signed": detect.GraspDetector(score_net, region_net, volume={"origin": ORIGIN}, approach=signed),
                 "retreat": detect.GraspDetector(score_net, region_net, volume={"origin": ORIGIN},
                                                 approach=dict(signed, retreat=True))}
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
    a, b = sorted(times["signed"]), sorted(times["retreat"])
    diff = statistics.median(b) - statistics.median(a)
    lines.append("GraspDetector.detect of two 640 x 480 views through the volume, approach in volume space, host clock, %d grasps of "
                 "grasp_stage3 analysed:" % len(out["grasp_stage3"]))
    lines.append("    --approach-signed --approach-field-cap 0.1                      %s" % fmt(a))
    lines.append("    --approach-signed --approach-field-cap 0.1 --approach-retreat   %s" % fmt(b))
    lines.append("    difference of the medians  %+9.3f ms = %+.2f%% of the frame time" % (diff, 100.0 * diff / statistics.median(a)))
    # That frame leaves the synthetic networks no grasp to analyse, so the stage is also timed where detect runs it
    # (_select_and_segment: the field of the frame, analyse_volume, the fan, the downloads) on FIXED proposals about the surface.
    B = 256
    surface = detectors["retreat"].fused
    k, _, _ = surface.check()
    cloud = surface.xyz[:k].cpu().numpy().astype(np.float64)
    transform = np.asarray(detectors["retreat"].transform if detectors["retreat"].table is None else detectors["retreat"].table[0],
                           dtype=np.float64)
    grng = np.random.default_rng(11)
    centres = cloud[grng.integers(0, k, B)] + grng.normal(0.0, 0.01, (B, 3))
    fixed = np.zeros((B, 8), dtype=np.float32)
    fixed[:, :3] = (centres @ transform[:3, :3].T + transform[:3, 3]).astype(np.float32)
    fixed[:, 3:6] = grng.standard_normal((B, 3))
    fixed[:, 6] = grng.uniform(-3.0, 3.0, B)
    fixed = torch.from_numpy(fixed).to(DEV)

    def stage(detector):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        _, extra, _ = detector._select_and_segment({"grasp_stage3": fixed}, None)
        host = {key: value.cpu().numpy() for key, value in extra.items()}
        return (time.perf_counter() - t0) * 1e3, host
    for _ in range(3):
        for detector in detectors.values():
            stage(detector)
    times = {name: [] for name in detectors}
    for _ in range(15):
        for name, detector in detectors.items():
            ms, host = stage(detector)
            times[name].append(ms)
    a, b = sorted(times["signed"]), sorted(times["retreat"])
    diff = statistics.median(b) - statistics.median(a)
    steps = host["grasp_retreat_steps"]
    lines.append("the detector's approach stage alone (the frame's field, analyse_volume, the downloads) on %d fixed proposals about "
                 "the surface, host clock:" % B)
    lines.append("    --approach-signed --approach-field-cap 0.1                      %s" % fmt(a))
    lines.append("    --approach-signed --approach-field-cap 0.1 --approach-retreat   %s" % fmt(b))
    lines.append("    difference of the medians  %+9.3f ms for the fan, the pick, their six record entries and downloads; %d of the "
                 "%d proposals have a free step, %d are free over the whole path" % (
                     diff, int((steps.max(axis=1) > 0).sum()), B, int((steps.max(axis=1) == steps.max()).sum())))
    return True


def run_step(name, path):
    import torch
    assert torch.cuda.is_available(), "this measurement needs the MI355X"
    lines = []
    ok = {"fan": step_fan, "detect": step_detect}[name](lines)
    with open(path, "w") as f:
        json.dump(lines, f)
    return 0 if ok else 1


def main():
    parser = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    parser.add_argument("--out", default=os.path.join(REPO, "profiles", "retreat_fan.txt"))
    parser.add_argument("--step", choices=[name for name, _ in STEPS], help="(internal) run one step in this process")
    parser.add_argument("--step-out", help="(internal) where the step leaves its lines")
    args = parser.parse_args()
    if args.step:
        sys.exit(run_step(args.step, args.step_out))
    import torch
    lines = ["retreat fan against the distance field of the TSDF volume (scripts/bench_retreat_fan.py): %s, torch %s" % (
        torch.cuda.get_device_name(0) if torch.cuda.is_available() else "no GPU", torch.__version__),
        "the two-view volume of scripts/bench_tsdf.py; gripper 8 cm x 6 cm, step = the 2 mm voxel; median of HIP-event times unless a "
        "host clock is named; the yardstick is the signed margin kernel on the same grasps in the same run (standoff %.2f m)" % STANDOFF,
        ""]
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
