"""What the signed, capped distance field of the TSDF volume costs on the MI355X (tsdf.Volume.distance_field(signed=,
max_distance=), regnet_tsdf_sdf in csrc/edt.hip) -> profiles/signed_field.txt.

Two steps, each a fresh child process under its own time limit; the driver stops at the first one that fails:
  field    the rendered two-view volume of scripts/bench_tsdf.py (320^3 voxels of 2 mm), both modes.  The yardstick is
           regnet_tsdf_edt, the path of the commit before the signed field, timed in the same run: its three passes singly
           (regnet_tsdf_edt_pass; the new entry has no single-pass form) and the whole call.  Beside it regnet_tsdf_sdf unsigned
           and signed, uncapped and capped at 5 cm and 10 cm, with and without ``nearest``, each with its ratio to the yardstick.
           Then ``query`` of 10^6 points -- the unsigned lookup, the signed nearest voxel, interpolated, interpolated with the
           gradient -- and the signed margin kernel at B = 16 and B = 4000 beside the unsigned one on the same grasps.
  detect   one GraspDetector.detect of the two-view MultiView in volume space with ``--approach-field`` against one with
           ``--approach-signed --approach-field-cap 0.1``, alternated.
Times are HIP events (field step) or a host clock around a call that ends in a download (detect step): warm-up first, then the
median of repeated runs with their min / max.  No time is gated.

    python scripts/bench_signed_field.py [--out profiles/signed_field.txt]
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
from bench_distance_field import DEPTH, DEV, STANDOFF, WIDTH, timed_after  # noqa: E402
from bench_outliers import fmt, timed  # noqa: E402
from bench_tsdf import ORIGIN, scene  # noqa: E402

STEPS = (("field", 540), ("detect", 420))       # (name, time limit in seconds)
CAPS_M = (None, 0.05, 0.10)


def step_field(lines):
    import numpy as np
    import torch
    from regnet_for_3d_grasping_amd import _lib, approach, eval_collision, tsdf
    mv, views = scene()
    params = tsdf.TsdfParams(origin=ORIGIN)
    vol = tsdf.Volume(params, DEV)
    for v in (0, 1):
        vol.integrate(views[v], mv.poses[v])
    surface = vol.extract()
    k, _, observed = surface.check()
    nx, ny, nz = params.dims
    n = nx * ny * nz
    lines.append("volume %d x %d x %d voxels of %g m, two views integrated: %d observed voxels, %d surface rows" % (
        params.dims + (params.voxel, observed, k)))
    med = statistics.median
    host_cloud = surface.xyz[:k].cpu().numpy()
    for mode in tsdf.FIELD_MODES:
        outside = mode == "solid_or_unseen"
        probe = vol.distance_field(mode, signed=True)
        inside = int((probe.dist2 < 0).sum())
        finite = probe.dist2[(probe.dist2 < 0) & (probe.dist2 > -tsdf.EDT_NONE)]
        deepest = float(-finite.min()) ** 0.5 if finite.numel() else float("inf")
        lines.append("mode %s, outside %d: %d obstacle voxels (%.2f%%), deepest obstacle voxel %.1f voxels from free space" % (
            mode, outside, inside, 100.0 * inside / n, deepest))
        del probe
        for nearest in (False, True):
            lines.append("  %s nearest" % ("with" if nearest else "without"))
            d2 = torch.empty((n,), dtype=torch.int32, device=DEV)
            near = torch.empty((n,), dtype=torch.int32, device=DEV) if nearest else None
            saved = [None, None]

            def one(p):
                _lib.call("regnet_tsdf_edt_pass", vol.data, vol.data.data_ptr(), nx, ny, nz, float(params.trunc),
                          int(params.min_weight), 0.0, tsdf.FIELD_MODES.index(mode), int(outside), p, d2.data_ptr(),
                          None if near is None else near.data_ptr())

            def restore():
                if saved[0] is not None:
                    d2.copy_(saved[0])
                    if nearest:
                        near.copy_(saved[1])

            for p, name in enumerate("xyz"):
                t = timed_after(restore, lambda: one(p), 2, 10)
                lines.append("    regnet_tsdf_edt_pass %s (the yardstick's)        %s" % (name, fmt(t)))
                restore()
                one(p)
                saved = [d2.clone(), near.clone() if nearest else None]
            del saved
            plain = vol.distance_field(mode, nearest=nearest)
            base = med(timed(lambda: vol.distance_field(mode, nearest=nearest, out=plain), 2, 10))
            lines.append("    regnet_tsdf_edt, the yardstick                  %9.3f ms" % base)
            del plain
            for signed in (False, True):
                field = vol.distance_field(mode, nearest=nearest, signed=signed, max_distance=0.05)
                for cap_m in CAPS_M:
                    if not signed and cap_m is None:

                        def call():                  # the new entry with sign = 0, cap = 0: the yardstick's bytes
                            _lib.call("regnet_tsdf_sdf", vol.data, vol.data.data_ptr(), nx, ny, nz, float(params.trunc),
                                      int(params.min_weight), 0.0, tsdf.FIELD_MODES.index(mode), int(outside), 0, 0,
                                      field.dist2.data_ptr(), field.nearest.data_ptr() if nearest else None, None)
                    else:

                        def call():
                            vol.distance_field(mode, nearest=nearest, signed=signed, max_distance=cap_m, out=field)
                    t = timed(call, 2, 10)
                    lines.append("    regnet_tsdf_sdf %-8s %-15s            %s   %.2fx of the yardstick" % (
                        "signed" if signed else "unsigned", "uncapped" if cap_m is None else "cap %g m (%d)" % (cap_m, field.cap),
                        fmt(t), med(t) / base))
                del field
            del d2, near
            torch.cuda.empty_cache()
        rng = np.random.default_rng(3)
        lo = np.asarray(ORIGIN)
        points = torch.from_numpy(rng.uniform(lo, lo + np.asarray(params.dims) * params.voxel, (1000000, 3)).astype(np.float32)).to(DEV)
        plain = vol.distance_field(mode, nearest=True)
        field = vol.distance_field(mode, nearest=True, signed=True, max_distance=0.10)
        t0 = timed(lambda: plain.query(points), 2, 10)
        t1 = timed(lambda: field.query(points), 2, 10)
        t2 = timed(lambda: field.query(points, interpolate=True), 2, 10)
        t3 = timed(lambda: field.query(points, interpolate=True, gradient=True), 2, 10)
        lines.append("  query of 10^6 uniform points: unsigned nearest voxel  %s" % fmt(t0))
        lines.append("                                signed nearest voxel    %s   %.2fx" % (fmt(t1), med(t1) / med(t0)))
        lines.append("                                signed interpolated     %s   %.2fx" % (fmt(t2), med(t2) / med(t0)))
        lines.append("                                ... with the gradient   %s   %.2fx" % (fmt(t3), med(t3) / med(t0)))
        t = timed(lambda: field.metres(), 2, 10)
        lines.append("  metres() of the whole signed field                    %s" % fmt(t))
        for B in (16, 4000):
            grasp = np.zeros((B, 8), dtype=np.float32)
            grng = np.random.default_rng(11)
            grasp[:, :3] = host_cloud[grng.integers(0, k, B)] + grng.normal(0.0, 0.01, (B, 3))
            grasp[:, 3:6] = grng.standard_normal((B, 3))
            grasp[:, 6] = grng.uniform(-3.0, 3.0, B)
            grasp = torch.from_numpy(grasp).to(DEV)
            res = approach.analyse_volume(vol, grasp, DEPTH, WIDTH, {"standoff": STANDOFF, "space": "volume"}, field=field)
            box, _ = eval_collision._box_args(DEPTH, WIDTH, B, grasp.device)
            margins = torch.empty((B, 2), dtype=torch.int32, device=DEV)
            counts = torch.empty((B, 6), dtype=torch.int32, device=DEV)

            def margin(name, plane):
                _lib.call(name, plane, plane.data_ptr(), nx, ny, nz, vol.origin.ctypes.data, float(params.voxel), int(outside),
                          res.L.data_ptr(), B, *box, STANDOFF, float(params.voxel), DEPTH, margins.data_ptr(), counts.data_ptr())

            t_u = timed(lambda: margin("regnet_grasp_margin_volume_f32", plain.dist2), 3, 20)
            t_s = timed(lambda: margin("regnet_grasp_margin_volume_signed_f32", field.dist2), 3, 20)
            lines.append("  B = %4d: regnet_grasp_margin_volume_f32          %s" % (B, fmt(t_u)))
            lines.append("            regnet_grasp_margin_volume_signed_f32   %s   %.2fx of the unsigned one" % (
                fmt(t_s), med(t_s) / med(t_u)))
            hand = res.margin_hand
            lines.append("            margin_hand: %d grasps below 0, deepest %.4f m, %d colliding hand samples" % (
                int((hand < 0).sum()), float(hand.min()), int(res.colliding_hand.sum())))
        del plain, field
        torch.cuda.empty_cache()
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
    detectors = {"field": detect.GraspDetector(score_net, region_net, volume={"origin": ORIGIN},
                                               approach={"space": "volume", "field": True}),
                 "signed": detect.GraspDetector(score_net, region_net, volume={"origin": ORIGIN}, approach=signed)}
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
    a, b = sorted(times["field"]), sorted(times["signed"])
    diff = statistics.median(b) - statistics.median(a)
    lines.append("GraspDetector.detect of two 640 x 480 views through the volume, approach in volume space, host clock, %d grasps of "
                 "grasp_stage3 analysed:" % len(out["grasp_stage3"]))
    lines.append("    --approach-field                                  %s" % fmt(a))
    lines.append("    --approach-signed --approach-field-cap 0.1        %s" % fmt(b))
    lines.append("    difference of the medians  %+9.3f ms = %+.2f%% of the frame time" % (diff, 100.0 * diff / statistics.median(a)))
    return True


def run_step(name, path):
    import torch
    assert torch.cuda.is_available(), "this measurement needs the MI355X"
    lines = []
    ok = {"field": step_field, "detect": step_detect}[name](lines)
    with open(path, "w") as f:
        json.dump(lines, f)
    return 0 if ok else 1


def main():
    parser = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    parser.add_argument("--out", default=os.path.join(REPO, "profiles", "signed_field.txt"))
    parser.add_argument("--step", choices=[name for name, _ in STEPS], help="(internal) run one step in this process")
    parser.add_argument("--step-out", help="(internal) where the step leaves its lines")
    args = parser.parse_args()
    if args.step:
        sys.exit(run_step(args.step, args.step_out))
    import torch
    lines = ["signed, capped distance field of the TSDF volume (scripts/bench_signed_field.py): %s, torch %s" % (
        torch.cuda.get_device_name(0) if torch.cuda.is_available() else "no GPU", torch.__version__),
        "the two-view volume of scripts/bench_tsdf.py; gripper 8 cm x 6 cm, standoff %.2f m, step = the 2 mm voxel; median of HIP-event "
        "times unless a host clock is named; the yardstick is regnet_tsdf_edt on the same volume in the same run" % STANDOFF, ""]
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
