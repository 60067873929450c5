"""What the hand-path check costs on the MI355X (approach.check_paths; regnet_grasp_path_check_signed_f32 in csrc/hand_path.hip)
-> profiles/hand_path.txt.

One step, a fresh child process under its own time limit: the rendered two-view volume of scripts/bench_tsdf.py (320^3 voxels
of 2 mm), its field signed and capped at 10 cm (mode solid).  At B = 16, 256 and 4000 grasps about the surface:
  * the path check with R = 5, K = 20 and TRANSLATION-ONLY paths -- the default fan's directions as ``straight_paths`` -- beside
    the retreat fan kernel on the same grasps, field and lattice, alternated in the same run.  By count the check makes the fan's
    lookups plus (K + 1) * 12 LDS reads per sample; the measured ratio is reported, and the share of profile words the two agree
    on (a path's pose is rounded once, the fan's sample position twice: they are not bit-equal under a general rotation);
  * the 9-path default (``default_paths``: the five directions and four turning paths), ``compose`` included separately.
Times are HIP events: warm-up first, then the median of repeated runs with their min / max.  No time is gated.

    python scripts/bench_hand_path.py [--out profiles/hand_path.txt]
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


def step_paths(lines):
    import numpy as np
    import torch
    from regnet_for_3d_grasping_amd import _lib, approach, eval_collision, hand_path, retreat, tsdf
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
    fan_params, path_params = retreat.RetreatParams(), hand_path.PathParams()
    R, K = 5, int(fan_params.steps)
    ds = float(fan_params.length) / K
    voxel = float(params.voxel)
    lines.append("field: mode solid, signed, capped at 0.10 m (%d voxels); R = %d, K = %d steps of %g m, tilt %g deg, lattice step = "
                 "the voxel; the 9-path default turns by %g deg" % (field.cap, R, K, ds, fan_params.tilt_deg, path_params.turn_deg))
    for B in SIZES:
        grasp = np.zeros((B, 8), dtype=np.float32)
        grng = np.random.default_rng(11)
        grasp[:, :3] = host_cloud[grng.integers(0, k, B)] + grng.normal(0.0, 0.01, (B, 3))
        grasp[:, 3:6] = grng.standard_normal((B, 3))
        grasp[:, 6] = grng.uniform(-3.0, 3.0, B)
        grasp = torch.from_numpy(grasp).to(DEV)
        fan = approach.retreat_fan(vol, field, grasp, DEPTH, WIDTH, fan_params)
        box, _ = eval_collision._box_args(DEPTH, WIDTH, B, grasp.device)
        local5 = hand_path.straight_paths(fan.dirs.cpu().numpy().astype(np.float64), float(fan_params.length), K)
        local9 = hand_path.default_paths(path_params)
        P5, P9 = hand_path.compose(fan.L, local5), hand_path.compose(fan.L, local9)
        f_profile, f_result = torch.empty_like(fan.profile), torch.empty_like(fan.result)
        outs = {}
        for name, P in (("5", P5), ("9", P9)):
            r = int(P.shape[1])
            outs[name] = (P, torch.empty((B, r, K + 1), dtype=torch.int32, device=DEV), torch.empty((B, r, 4), dtype=torch.int32, device=DEV),
                          torch.empty((B, r, K), dtype=torch.float32, device=DEV))

        def kernel_fan():
            _lib.call("regnet_grasp_retreat_fan_signed_f32", field.dist2, field.dist2.data_ptr(), nx, ny, nz,
                      vol.origin.ctypes.data, voxel, 0, fan.L.data_ptr(), B, *box, voxel, DEPTH, fan.dirs.data_ptr(), 0, R, K, ds,
                      fan.thresh, f_profile.data_ptr(), f_result.data_ptr())

        def kernel_check(name):
            P, profile, result, disp = outs[name]
            _lib.call("regnet_grasp_path_check_signed_f32", field.dist2, field.dist2.data_ptr(), nx, ny, nz,
                      vol.origin.ctypes.data, voxel, 0, P.data_ptr(), B, int(P.shape[1]), K, *box, voxel, DEPTH, fan.thresh,
                      profile.data_ptr(), result.data_ptr(), disp.data_ptr())

        t_f, t_c = [], []
        for _ in range(4):                           # alternated: both see the same neighbours on the machine
            t_f += timed(kernel_fan, 2, 5)
            t_c += timed(lambda: kernel_check("5"), 2, 5)
        t_f, t_c = sorted(t_f), sorted(t_c)
        t_9 = timed(lambda: kernel_check("9"), 3, 20)
        t_compose = timed(lambda: hand_path.compose(fan.L, local9), 3, 20)
        assert torch.equal(f_profile, fan.profile)
        same = float((outs["5"][1] == f_profile).to(torch.float32).mean())
        lines.append("B = %4d: regnet_grasp_retreat_fan_signed_f32 (yardstick), R = 5, K = 20     %s" % (B, fmt(t_f)))
        lines.append("          regnet_grasp_path_check_signed_f32, 5 translation-only paths      %s   %.2fx of the fan; %.2f%% of the "
                     "profile words equal the fan's" % (fmt(t_c), med(t_c) / med(t_f), 100.0 * same))
        lines.append("          regnet_grasp_path_check_signed_f32, the 9 default paths           %s   %.2fx of the fan, %.2fx of the "
                     "5-path check (9 / 5 = 1.80 by count)" % (fmt(t_9), med(t_9) / med(t_f), med(t_9) / med(t_c)))
        lines.append("          compose (B,12) x (9,K+1,12) -> P of %.2f MB, torch float64           %s" % (
            outs["9"][0].numel() * 4e-6, fmt(t_compose)))
        check = approach.check_paths(vol, field, grasp, DEPTH, WIDTH, path_params, rows=(fan.frame, fan.center, fan.L))
        assert torch.equal(check.profile, outs["9"][1]) and torch.equal(check.disp, outs["9"][3])
        steps, index, certified = check.free_steps.cpu().numpy(), check.index.cpu().numpy(), check.certified_steps().cpu().numpy()
        lines.append("          the 9 default paths: %d of %d grasps have a free step on some path, the pick takes a turning path for %d; "
                     "%d free steps in all, %d of them certified at the default slack" % (
                         int((steps.max(axis=1) > 0).sum()), B, int((index >= 5).sum()), int(steps.sum()), int(certified.sum())))
    return True


def run_step(path):
    import torch
    assert torch.cuda.is_available(), "this measurement needs the MI355X"
    lines = []
    ok = step_paths(lines)
    with open(path, "w") as f:
        json.dump(lines, f)
    return 0 if ok else 1


def main():
    parser = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    parser.add_argument("--out", default=os.path.join(REPO, "profiles", "hand_path.txt"))
    parser.add_argument("--step", action="store_true", help="(internal) run the step in this process")
    parser.add_argument("--step-out", help="(internal) where the step leaves its lines")
    args = parser.parse_args()
    if args.step:
        sys.exit(run_step(args.step_out))
    import torch
    lines = ["hand paths against the distance field of the TSDF volume (scripts/bench_hand_path.py): %s, torch %s" % (
        torch.cuda.get_device_name(0) if torch.cuda.is_available() else "no GPU", torch.__version__),
        "the two-view volume of scripts/bench_tsdf.py; gripper 8 cm x 6 cm, step = the 2 mm voxel; medians of HIP-event times; the "
        "yardstick is the retreat fan kernel on the same grasps, field and lattice in the same run, alternated with the check", ""]
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
