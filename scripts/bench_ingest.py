"""Single-frame front end (csrc/ingest.hip + the device draws) against the reference's host front end, on one 640 x 480
frame with 30 % holes (the frame of tests/test_gpu_ingest.py's crop test).

  device : HIP-event time of ingest.ingest_frame -- crop + rand(3) + choice + resample -- with the frame already in HBM, the
           same including the upload of the float64 frame, and the split by step (events between the steps);
  host   : wall time of the numpy restatement of test.py:112-127 (tests/ingest_reference.py) followed by the upload of its
           (25600, 6) result;
  detect : wall time of GraspDetector.detect with each front end (seeded, calibrated synthetic networks).
Three fresh processes per front end, alternating, 20 timed calls after 5 warm-up calls each; median and range per process.
The numbers describe the feature; they gate nothing.

    python scripts/bench_ingest.py [profiles/ingest.json]
"""
import json
import os
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
WARMUP, CALLS, PROCESSES = 5, 20, 3
CHILD_TIMEOUT = 240


def _stats(ms):
    ms = sorted(ms)
    return {"median": ms[len(ms) // 2], "min": ms[0], "max": ms[-1]}


def child(kind):
    import numpy as np
    import torch
    from regnet_for_3d_grasping_amd import detect, ingest, np_random, pipeline, synthetic
    from regnet_for_3d_grasping_amd.get_regiondataset import get_grasp_allobj
    from tests import ingest_reference as ir
    dev = torch.device("cuda:0")
    T = ingest.table_frame_transform()
    xyz, rgb = ir.camera_frame(11, 640 * 480, T)
    out = {"kind": kind, "points": int(len(xyz))}

    def event():
        e = torch.cuda.Event(enable_timing=True)
        e.record()
        return e

    def host_front_end():
        pc, back, color = ir.resample(ir.crop(xyz, rgb, T)[0])
        return torch.from_numpy(pc).view(1, -1, 6).to(dev), back, color

    np.random.seed(1)
    if kind == "device":
        xyz_d, rgb_d = torch.from_numpy(xyz).to(dev), torch.from_numpy(rgb).to(dev)
        resident, with_upload, steps = [], [], {"crop": [], "rand3": [], "choice": [], "resample": []}
        with np_random.deferred():
            for it in range(WARMUP + CALLS):
                a = event()
                fr = ingest.ingest_frame(xyz_d, rgb_d, T, device=dev)
                b = event()
                fr = ingest.ingest_frame(xyz, rgb, T, device=dev)
                c = event()
                # the same steps one by one, an event between them
                e0 = event()
                k64, k32, krgb, count, _ = ingest.crop_frame(xyz_d, rgb_d, T)
                e1 = event()
                rand3 = np_random.rand_device(3, dev)
                e2 = event()
                pick = np_random.choice_rows_device(count, 25600, 0, len(xyz))[0].view(-1)
                e3 = event()
                pc = torch.empty((25600, 6), dtype=torch.float32, device=dev)
                bad = torch.zeros((1,), dtype=torch.int32, device=dev)
                ingest._lib.check(ingest._L.regnet_ingest_resample_f32(k32.data_ptr(), krgb.data_ptr(), 1, count.data_ptr(), len(xyz),
                                                                       pick.data_ptr(), 25600, rand3.data_ptr(), pc.data_ptr(),
                                                                       bad.data_ptr(), torch.cuda.current_stream(dev).cuda_stream),
                                  "ingest_resample")
                e4 = event()
                torch.cuda.synchronize()
                if it >= WARMUP:
                    resident.append(a.elapsed_time(b))
                    with_upload.append(b.elapsed_time(c))
                    for name, (s, e) in zip(steps, ((e0, e1), (e1, e2), (e2, e3), (e3, e4))):
                        steps[name].append(s.elapsed_time(e))
            out["kept"] = int(fr.count.cpu())
        out["front_end_ms"] = _stats(resident)
        out["front_end_with_upload_ms"] = _stats(with_upload)
        out["steps_ms"] = {name: _stats(v) for name, v in steps.items()}
    else:
        wall = []
        for it in range(WARMUP + CALLS):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            pc, back, _ = host_front_end()
            torch.cuda.synchronize()
            if it >= WARMUP:
                wall.append((time.perf_counter() - t0) * 1e3)
        out["kept"] = int(len(back))
        out["front_end_ms"] = _stats(wall)

    # ---- detect() with this front end (a failure of the synthetic calibration on this frame is recorded, not fatal)
    try:
        score_net, region_net = pipeline.build_models(dev)
        score_net.eval()
        region_net.eval()
        np.random.seed(2)
        pc, back, color = host_front_end()
        synthetic.calibrate_score_head(score_net, pc)
        with torch.no_grad():
            feat, score, _ = score_net(pc)
        g = get_grasp_allobj(pc, score, detect.TEST_PARAMS, [], True)
        import contextlib
        import io

        def run():
            with contextlib.redirect_stdout(io.StringIO()), torch.no_grad():
                return region_net(g[3], g[5], g[2], g[4], g[0], g[1], pc, feat, detect.GRIPPER_PARAMS, None, [])
        synthetic.calibrate_region_head(region_net, run)
        detector = detect.GraspDetector(score_net, region_net, transform=T)
        wall = []
        for it in range(WARMUP + CALLS):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            if kind == "device":
                res = detector.detect((xyz, rgb))
            else:
                pc, back, color = host_front_end()
                n = len(back)
                frame = ingest.Frame(pc, torch.from_numpy(back).to(dev), torch.from_numpy(color).to(dev),
                                     torch.from_numpy(back.astype(np.float32)).to(dev),
                                     torch.full((1,), n, dtype=torch.int32, device=dev),
                                     torch.zeros((1,), dtype=torch.int32, device=dev))
                res = detector.detect(frame)
            torch.cuda.synchronize()
            if it >= WARMUP:
                wall.append((time.perf_counter() - t0) * 1e3)
        out["detect_wall_ms"] = _stats(wall)
        out["detect_grasps"] = {k: int(len(res[k])) for k in res if k.startswith("grasp")}
    except Exception as exc:      # noqa: BLE001
        out["detect_error"] = "%s: %s" % (type(exc).__name__, exc)
    print("RESULT " + json.dumps(out), flush=True)


def main():
    runs = []
    for i in range(PROCESSES):
        for kind in ("device", "host"):
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", kind], stdout=subprocess.PIPE,
                               stderr=subprocess.PIPE, timeout=CHILD_TIMEOUT)
            if p.returncode != 0:           # a failed or faulted child ends the measurement: nothing more is started
                sys.stderr.write(p.stderr.decode(errors="replace")[-4000:])
                raise SystemExit("bench_ingest: child %s exited with %d" % (kind, p.returncode))
            line = [ln for ln in p.stdout.decode().splitlines() if ln.startswith("RESULT ")][-1]
            runs.append(json.loads(line[len("RESULT "):]))
            print(line, flush=True)
    res = {"frame": "640 x 480, 30 % NaN rows, float64", "unit": "ms", "warmup": WARMUP, "calls": CALLS, "runs": runs}
    for kind in ("device", "host"):
        med = [r["front_end_ms"]["median"] for r in runs if r["kind"] == kind]
        res[kind + "_front_end_median_of_medians"] = sorted(med)[len(med) // 2]
        res[kind + "_front_end_range_of_medians"] = [min(med), max(med)]
    print(json.dumps({k: v for k, v in res.items() if k != "runs"}))
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--child":
        child(sys.argv[2])
    else:
        main()
