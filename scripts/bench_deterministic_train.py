"""Cost of the deterministic mode (torch.use_deterministic_algorithms(True)) at configs[3]'s training shape, 8 x 25 600.

Records, into profiles/deterministic_train.json:
  * the RefineTrainer iteration (wall time per iteration over the timed steps, after warm-up) with the mode off and on,
    same box, alternating runs, each run a fresh child process under its own `timeout`;
  * the new kernels against the default ones they replace, from HIP events (median of 5 after one warm-up call): the sort
    plan and segment sums of the level-2 / level-3 grouping backwards and of the FP blocks' interpolation backwards, the
    BatchNorm passes of a level-2 layer, scatter_max_grad.

    python scripts/bench_deterministic_train.py [--pairs 2] [--steps 10] [--warmup 4] [--out profiles/deterministic_train.json]
"""
import argparse
import json
import os
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
B, N = 8, 25600


def child_train(mode, steps, warmup):
    import numpy as np
    import torch
    from regnet_for_3d_grasping_amd import pipeline, synthetic
    from regnet_for_3d_grasping_amd.gripper_region_network import GripperRegionNetwork
    from regnet_for_3d_grasping_amd.score_network import ScoreNetwork
    from regnet_for_3d_grasping_amd.train_step import RefineTrainer
    torch.use_deterministic_algorithms(mode == "on")
    dev = torch.device("cuda:0")
    pc = torch.from_numpy(np.stack([synthetic.make_scene(1000 + b, N) for b in range(B)], 0))
    records = [synthetic.make_grasp_labels(pc[b].numpy(), 1050 + b) for b in range(B)]
    target = torch.from_numpy(np.random.default_rng(2).uniform(0, 1, (B, N)).astype(np.float32)).to(dev)
    pc = pc.to(dev)
    score_net = ScoreNetwork(training=True)
    score_net.load_state_dict(synthetic.seeded_state_dict(score_net, 7))
    region_net = GripperRegionNetwork(training=True, group_num=pipeline.GROUP_NUM, gripper_num=pipeline.GRIPPER_NUM,
                                      grasp_score_threshold=pipeline.GRASP_SCORE_THRESHOLD, radius=pipeline.DEPTH,
                                      reg_channel=pipeline.REG_CHANNEL)
    region_net.load_state_dict(synthetic.seeded_state_dict(region_net, 11))
    synthetic.set_region_head_affine(region_net)
    trainer = RefineTrainer(score_net.to(dev), region_net.to(dev), pipeline.PARAMS, pipeline.GRIPPER_PARAMS)
    np.random.seed(0)
    for _ in range(warmup):
        trainer.step(pc, target, records)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        trainer.step(pc, target, records)
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) * 1e3 / steps
    return {"mode": mode, "ms_per_iteration": round(ms, 3), "steps": steps, "warmup": warmup,
            "graph_replays": trainer.graph_replays}


def _timed(fn, reps=5):
    import torch
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return round(sorted(ts)[len(ts) // 2], 4)


def child_kernels():
    import torch
    from regnet_for_3d_grasping_amd import bn_train, pn2_ext, region_ops, synthetic
    dev = torch.device("cuda:0")
    L_ = pn2_ext._L
    st = lambda: torch.cuda.current_stream(dev).cuda_stream   # noqa: E731
    pc = synthetic.make_batch(1000, B, N).to(dev)
    clouds, tables = [pc[:, :, :3].transpose(1, 2).contiguous()], []     # (B, N, 6) scenes -> (B, 3, N)
    for M, r in ((5120, 0.02), (1024, 0.08), (256, 0.32)):
        src = clouds[-1]
        cent = pn2_ext.gather_points(src, pn2_ext.farthest_point_sample(src, M)).contiguous()
        tables.append((pn2_ext.ball_query(src, cent, r, 64)[0], src.shape[2]))
        clouds.append(cent)
    out = {}

    def both(name, default, det):
        torch.use_deterministic_algorithms(False)
        d = _timed(default)
        torch.use_deterministic_algorithms(True)
        e = _timed(det)
        torch.use_deterministic_algorithms(False)
        out[name] = {"default_ms": d, "deterministic_ms": e}

    # grouping backward of the pre-multiplied first layers (levels 2 and 3: C1 = 256 / 512)
    for (idx, n1), C, name in ((tables[1], 256, "group_bwd_level2"), (tables[2], 512, "group_bwd_level3")):
        g = torch.randn((B, C) + tuple(idx.shape[1:]), device=dev)
        both(name, lambda: pn2_ext.group_points_backward(g, idx, n1), lambda: pn2_ext.group_points_backward(g, idx, n1))
        plan = pn2_ext.scatter_plan(idx, n1)
        out[name]["plan_ms"] = _timed(lambda: pn2_ext.scatter_plan(idx, n1))
        gi = torch.empty((B, C, n1), device=dev)
        L = idx[0].numel()
        out[name]["segsum_ms"] = _timed(lambda: L_.regnet_scatter_segsum_f32(
            g.data_ptr(), *g.stride(), idx.shape[2], None, B, C, n1, L, plan.buffer.data_ptr(), gi.data_ptr(), st()))
    # interpolation backward of the FP blocks' pre-multiplied layers (sparse M, dense N, C1)
    for dense, sparse, C, name in ((clouds[2], clouds[3], 1024, "interp_bwd_fp1"), (clouds[1], clouds[2], 512, "interp_bwd_fp2"),
                                   (clouds[0], clouds[1], 256, "interp_bwd_fp3")):
        idx, d2 = pn2_ext.point_search(dense, sparse, 3)
        w = (1.0 / (d2 + 1e-8))
        w = (w / w.sum(2, keepdim=True)).contiguous()
        g = torch.randn(B, C, dense.shape[2], device=dev)
        m = sparse.shape[2]
        both(name, lambda: pn2_ext.interpolate_backward(g, idx, w, m), lambda: pn2_ext.interpolate_backward(g, idx, w, m))
    # BatchNorm passes of a level-2 layer: (8, 256, 1024 x 64), pooled over the 64 neighbours and not
    bn = torch.nn.BatchNorm2d(256).to(dev).train()
    x = torch.randn(B, 256, 1024, 64, device=dev)
    dy = torch.randn(B, 256, 1024, 64, device=dev)
    both("bn_stats_level2", lambda: bn_train.bn_stats(bn, x), lambda: bn_train.bn_stats(bn, x))
    xg = x.clone().requires_grad_(True)

    def fwd_bwd():
        y = bn_train.bn_relu(bn, xg, True)
        torch.autograd.grad(y, xg, dy)
    both("bn_relu_fwd_bwd_level2", fwd_bwd, fwd_bwd)
    # the pooled region feature's backward: R x F
    R, F, rows = 2048, 256, B * N
    arg = torch.randint(0, rows, (R, F), device=dev)
    dyr = torch.randn(R, F, device=dev)
    grad = torch.zeros(rows, F, device=dev)
    both("scatter_max_grad", lambda: region_ops._scatter_max_grad(dyr, arg, grad, rows, 0, F, 1),
         lambda: region_ops._scatter_max_grad(dyr, arg, grad, rows, 0, F, 1))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=2)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--timeout", type=int, default=900, help="seconds per child run")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "deterministic_train.json"))
    ap.add_argument("--child", choices=["off", "on", "kernels"])
    args = ap.parse_args()
    if args.child:
        res = child_kernels() if args.child == "kernels" else child_train(args.child, args.steps, args.warmup)
        print("RESULT " + json.dumps(res))
        return
    runs = []
    plan = [m for _ in range(args.pairs) for m in ("off", "on")] + ["kernels"]
    for mode in plan:
        cmd = ["timeout", "-k", "10", str(args.timeout), sys.executable, os.path.abspath(__file__), "--child", mode,
               "--steps", str(args.steps), "--warmup", str(args.warmup)]
        p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, cwd=REPO)
        text = p.stdout.decode(errors="replace")
        lines = [l for l in text.splitlines() if l.startswith("RESULT ")]
        if p.returncode != 0 or not lines:
            print(text[-3000:])
            raise SystemExit("child %s ended with status %d" % (mode, p.returncode))
        res = json.loads(lines[-1][len("RESULT "):])
        print(mode, res)
        runs.append(res)
    train = [r for r in runs if "mode" in r]
    off = [r["ms_per_iteration"] for r in train if r["mode"] == "off"]
    on = [r["ms_per_iteration"] for r in train if r["mode"] == "on"]
    report = {
        "what": "RefineTrainer iteration at 8 x 25 600 (configs[3]), deterministic mode off / on, alternating fresh processes; "
                "new kernels vs the default ones (HIP events, median of 5)",
        "iteration_ms": {"off": off, "on": on, "off_median": sorted(off)[len(off) // 2], "on_median": sorted(on)[len(on) // 2]},
        "runs": train,
        "kernels_ms": runs[-1],
    }
    report["iteration_ms"]["on_over_off"] = round(report["iteration_ms"]["on_median"] / report["iteration_ms"]["off_median"], 4)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(report, f, indent=1)
    print(json.dumps(report["iteration_ms"]))


if __name__ == "__main__":
    main()
