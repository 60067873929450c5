"""What the push-out costs on the MI355X (approach.push_out; regnet_grasp_push_out_f32 in csrc/hand_adjust.hip)
-> profiles/push_out.txt.

One step, a fresh child process under its own time limit: the rendered two-view volume of scripts/bench_tsdf.py (320^3 voxels
of 2 mm), its field signed and capped at 10 cm (mode solid).  At B = 16, 256 and 4000 grasps about the surface:
  * the push-out with the default parameters and with 64 iterations, beside regnet_grasp_margin_volume_signed_f32 on the same
    grasps, field and lattice step (standoff 0), alternated in the same run: the margin kernel makes ONE nearest-voxel lookup per
    sample, the push-out eight loads per hand sample per iterate;
  * ONE iterate of the same method written in torch operations -- the hand samples through ``L``, ``field.query(interpolate=True,
    gradient=True)`` on them, ``amin`` per grasp -- at B = 16 and 256 (at 4000 its intermediates do not fit a sensible budget).
Times are HIP events: warm-up first, then the median of repeated runs with their min / max.  No time is gated.

    python scripts/bench_push_out.py [--out profiles/push_out.txt]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_distance_field import DEPTH, DEV, WIDTH  # noqa: E402
from bench_outliers import fmt, timed  # noqa: E402
from bench_tsdf import ORIGIN, scene  # noqa: E402

LIMIT = 420                                     # the step's time limit in seconds
SIZES = (16, 256, 4000)
TORCH_SIZES = (16, 256)


def hand_points(box, step, x_extent):
    """The hand's samples of the fan's lattice in the local frame -> (n,3) float32 (host), by the contract's rules."""
    import numpy as np
    from regnet_for_3d_grasping_amd import approach_volume
    x_lo, x_hi, ht, hw, hs, back_x = (np.float32(v) for v in box[:2] + box[3:])
    n_x, n_y, n_z = approach_volume.lattice(box, 0.0, step, x_extent)
    h = np.float32(step)
    x = x_lo + (np.arange(n_x, dtype=np.float32) + np.float32(0.5)) * h
    y = (np.arange(n_y, dtype=np.float32) + np.float32(0.5)) * h - hw
    z = (np.arange(n_z, dtype=np.float32) + np.float32(0.5)) * h - ht
    x, y, z = (a.reshape(-1) for a in np.meshgrid(x, y, z, indexing="ij"))
    section = (z < ht) & (z > -ht) & (y < hw) & (y > -hw)
    close = (x > x_lo) & (x < x_hi)
    hand = section & close & ((x < back_x) | (y > hs) | (y < -hs))
    return np.stack([x[hand], y[hand], z[hand]], axis=1)


def step_push(lines):
    import numpy as np
    import torch
    from regnet_for_3d_grasping_amd import _lib, approach, approach_volume, eval_collision, hand_adjust, tsdf
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
    voxel = float(params.voxel)
    default, long = hand_adjust.PushParams(), hand_adjust.PushParams(iterations=64)
    lines.append("field: mode solid, signed, capped at 0.10 m (%d voxels); target %g m, max_shift %g m, axes 1 1 1, lattice step = the "
                 "voxel; %d iterations (the default) and 64" % (field.cap, default.target, default.max_shift, default.iterations))
    for B in SIZES:
        grasp = np.zeros((B, 8), dtype=np.float32)
        grng = np.random.default_rng(11)
        grasp[:, :3] = host_cloud[grng.integers(0, k, B)] + grng.normal(0.0, 0.01, (B, 3))
        grasp[:, 3:6] = grng.standard_normal((B, 3))
        grasp[:, 6] = grng.uniform(-3.0, 3.0, B)
        grasp = torch.from_numpy(grasp).to(DEV)
        _, frame, center, L = approach_volume.local_to_volume(grasp, None)
        box, _ = eval_collision._box_args(DEPTH, WIDTH, B, grasp.device)
        margins = torch.empty((B, 2), dtype=torch.int32, device=DEV)
        counts = torch.empty((B, 6), dtype=torch.int32, device=DEV)

        def kernel_margin():
            _lib.call("regnet_grasp_margin_volume_signed_f32", field.dist2, field.dist2.data_ptr(), nx, ny, nz,
                      vol.origin.ctypes.data, voxel, 0, L.data_ptr(), B, *box, 0.0, voxel, DEPTH, margins.data_ptr(), counts.data_ptr())

        def push(p):
            return approach.push_out(vol, field, grasp, DEPTH, WIDTH, p, rows=(frame, center, L))

        t_m, t_p = [], []
        for _ in range(4):                           # alternated: both see the same neighbours on the machine
            t_m += timed(kernel_margin, 2, 5)
            t_p += timed(lambda: push(default), 2, 5)
        t_m, t_p = sorted(t_m), sorted(t_p)
        t_64 = timed(lambda: push(long), 3, 20)
        out, out64 = push(default), push(long)
        status, status64 = out.status.cpu().numpy(), out64.status.cpu().numpy()
        lines.append("B = %4d: regnet_grasp_margin_volume_signed_f32 (yardstick), standoff 0       %s" % (B, fmt(t_m)))
        lines.append("          push_out, %2d iterations (the wrapper's allocations included)       %s   %.2fx of the margin" % (
            default.iterations, fmt(t_p), med(t_p) / med(t_m)))
        lines.append("          push_out, 64 iterations                                             %s   %.2fx of the margin" % (
            fmt(t_64), med(t_64) / med(t_m)))
        for name, st, o in (("%2d" % default.iterations, status, out), ("64", status64, out64)):
            lines.append("          %s iterations: %s; %d steps applied in all" % (
                name, ", ".join("%s %d" % (hand_adjust.STATUS[s], int((st == s).sum())) for s in range(6)), int(o.iterations.sum())))
        if B in TORCH_SIZES:
            local = torch.from_numpy(hand_points(box, voxel, DEPTH)).to(DEV)
            rows = L.view(B, 3, 4)

            def torch_iterate():
                world = torch.einsum("bij,nj->bni", rows[:, :, :3], local) + rows[:, None, :, 3]
                value, gradient = field.query(world.reshape(-1, 3), interpolate=True, gradient=True)
                value = torch.nan_to_num(value.view(B, -1), nan=float("inf"))
                low = value.amin(dim=1)
                at = value.argmin(dim=1)
                g = gradient.view(B, -1, 3)[torch.arange(B, device=DEV), at]
                return low, torch.einsum("bij,bi->bj", rows[:, :, :3], g)

            t_t = timed(torch_iterate, 3, 20)
            lines.append("          ONE iterate in torch operations (%d hand samples per grasp: apply L, field.query with the gradient, "
                         "amin, argmin, gather, rotate)   %s   %.2fx of the %d-iteration push_out" % (
                             int(local.shape[0]), fmt(t_t), med(t_t) / med(t_p), default.iterations))
    return True


def run_step(path):
    import torch
    assert torch.cuda.is_available(), "this measurement needs the MI355X"
    lines = []
    ok = step_push(lines)
    with open(path, "w") as f:
        json.dump(lines, f)
    return 0 if ok else 1


def main():
    parser = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    parser.add_argument("--out", default=os.path.join(REPO, "profiles", "push_out.txt"))
    parser.add_argument("--step", action="store_true", help="(internal) run the step in this process")
    parser.add_argument("--step-out", help="(internal) where the step leaves its lines")
    args = parser.parse_args()
    if args.step:
        sys.exit(run_step(args.step_out))
    import torch
    lines = ["push-out along the signed distance field of the TSDF volume (scripts/bench_push_out.py): %s, torch %s" % (
        torch.cuda.get_device_name(0) if torch.cuda.is_available() else "no GPU", torch.__version__),
        "the two-view volume of scripts/bench_tsdf.py; gripper 8 cm x 6 cm, step = the 2 mm voxel; medians of HIP-event times; the "
        "yardstick is the signed margin kernel on the same grasps, field and lattice step in the same run, alternated with the push-out", ""]
    part = args.out + ".step.json"
    try:
        status = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", "--step-out", part], timeout=LIMIT).returncode
    except subprocess.TimeoutExpired:
        status = 124
    if os.path.exists(part):
        with open(part) as f:
            lines += json.load(f) + [""]
        os.remove(part)
    if status != 0:
        lines.append("the step ended with status %d" % status)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines).rstrip() + "\n")
    print("\n".join(lines))
    sys.exit(status)


if __name__ == "__main__":
    main()
