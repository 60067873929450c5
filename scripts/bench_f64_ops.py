"""Wall time of the float64 operators (csrc/ops_f64.hip, scatter.hip) at configs[2]'s shapes -- 8 scenes x 25 600
points, levels of 5 120 / 1 024 / 256 centroids -- and of one ``.double()`` ScoreNetwork forward (eval, no_grad) at
8 x 25 600.  The float64 path is a correctness / compatibility path; these numbers describe it, they gate nothing.

    python scripts/bench_f64_ops.py [out.json]        (HIP events, median of 5 after one warm-up call)
"""
import json
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from regnet_for_3d_grasping_amd import dgcnn_ext, pn2_ext, synthetic  # noqa: E402
from regnet_for_3d_grasping_amd.score_network import ScoreNetwork  # noqa: E402

DEV = torch.device("cuda:0")
B, N = 8, 25600
LEVELS = [(25600, 5120, 0.02, 3), (5120, 1024, 0.08, 256), (1024, 256, 0.32, 512)]   # (points, centroids, radius, C in)
FP = [(256, 1024, 1024), (1024, 5120, 256), (5120, 25600, 256)]                        # (sparse, dense, C sparse)


def timed(fn, reps=5):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    return sorted(ts)[len(ts) // 2]


def main():
    torch.manual_seed(0)
    pc = synthetic.make_batch(1000, B, N).double().to(DEV)
    xyz = pc[:, :, :3].transpose(1, 2)                       # the (B, 3, N) view ScoreNet hands the operators
    res = {"device": torch.cuda.get_device_name(0), "B": B, "N": N, "unit": "ms", "ops": []}
    pts = xyz
    for (n, m, r, c) in LEVELS:
        ctr = pn2_ext.farthest_point_sample(pts, m)
        cxyz = torch.gather(pts, 2, ctr[:, None, :].expand(B, 3, m))
        idx, _ = pn2_ext.ball_query(pts, cxyz, r, 64)
        feat = torch.randn(B, c, n, dtype=torch.float64, device=DEV)
        grad = torch.randn(B, c, m, 64, dtype=torch.float64, device=DEV)
        row = {"level": "%d -> %d" % (n, m), "C": c,
               "fps": timed(lambda: pn2_ext.farthest_point_sample(pts, m), reps=3),
               "ball_query": timed(lambda: pn2_ext.ball_query(pts, cxyz, r, 64)),
               "group_fwd": timed(lambda: pn2_ext.group_points_forward(feat, idx)),
               "group_bwd": timed(lambda: pn2_ext.group_points_backward(grad, idx, n)),
               "gather_knn_fwd": timed(lambda: dgcnn_ext.gather_knn_forward(feat, idx))}
        res["ops"].append(row)
        print(json.dumps(row), flush=True)
        pts = cxyz
    for (ns, nd, c) in FP:
        sp = torch.rand(B, 3, ns, dtype=torch.float64, device=DEV)
        de = torch.rand(B, 3, nd, dtype=torch.float64, device=DEV)
        idx, d2 = pn2_ext.point_search(de, sp, 3)
        w = (1.0 / d2.clamp(min=1e-10))
        w = w / w.sum(2, keepdim=True)
        feat = torch.randn(B, c, ns, dtype=torch.float64, device=DEV)
        grad = torch.randn(B, c, nd, dtype=torch.float64, device=DEV)
        row = {"level": "%d -> %d" % (ns, nd), "C": c,
               "three_nn": timed(lambda: pn2_ext.point_search(de, sp, 3)),
               "interp_fwd": timed(lambda: pn2_ext.interpolate_forward(feat, idx, w)),
               "interp_bwd": timed(lambda: pn2_ext.interpolate_backward(grad, idx, w, ns))}
        res["ops"].append(row)
        print(json.dumps(row), flush=True)
    net = ScoreNetwork(training=False).double().to(DEV).eval()
    with torch.no_grad():
        res["score_network_forward_double"] = timed(lambda: net(pc), reps=3)
    print(json.dumps({"score_network_forward_double": res["score_network_forward_double"]}), flush=True)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
