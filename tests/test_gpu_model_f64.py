"""A ``.double()`` ScoreNetwork / PointNet2Seg on the MI355X: the float64 operator path (csrc/ops_f64.hip + torch's own
dense layers) against the same module on the CPU in double with pn2_ext / dgcnn_ext swapped for tests/f64_reference.py.
The geometry (every level's sampling, ball-query and 3-NN indices) must agree exactly; scores, losses and gradients
differ only in the dense layers' float64 summation order.  The float32-only stages refuse float64 input."""
import contextlib

import pytest
import torch

from . import f64_reference as R

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
B, N = 2, 6144


class _Recorder:
    """Proxy of a pn2_ext-like module that records the index outputs of the geometry ops."""

    def __init__(self, inner):
        self.inner, self.log = inner, []

    def __getattr__(self, name):
        fn = getattr(self.inner, name)
        if name not in ("farthest_point_sample", "ball_query", "point_search"):
            return fn

        def rec(*args, **kwargs):
            out = fn(*args, **kwargs)
            idx = out if isinstance(out, torch.Tensor) else out[0]
            self.log.append((name, idx.detach().cpu()))
            return out
        return rec


@contextlib.contextmanager
def backend(ext, knn):
    """pn2_ext / dgcnn_ext of the operator layer swapped for ``ext`` / ``knn`` (the oracle_backend pattern)."""
    import regnet_for_3d_grasping_amd.pn2_utils.function as fn
    import regnet_for_3d_grasping_amd.pn2_utils.functions.gather_knn as gk
    saved = fn.pn2_ext, gk.dgcnn_ext
    fn.pn2_ext, gk.dgcnn_ext = ext, knn
    try:
        yield
    finally:
        fn.pn2_ext, gk.dgcnn_ext = saved


def _gpu_backend():
    from regnet_for_3d_grasping_amd import dgcnn_ext, pn2_ext
    return _Recorder(pn2_ext), dgcnn_ext


def _cpu_backend():
    return _Recorder(R), R


@pytest.fixture(scope="module")
def nets():
    from regnet_for_3d_grasping_amd import synthetic
    from regnet_for_3d_grasping_amd.score_network import ScoreNetwork
    torch.manual_seed(0)
    cpu = ScoreNetwork(training=True)
    cpu.extrat_featurePN2.mlp.dropout_prob = 0.0
    cpu = cpu.double()
    gpu = ScoreNetwork(training=True)
    gpu.extrat_featurePN2.mlp.dropout_prob = 0.0
    gpu.load_state_dict(cpu.state_dict())
    gpu = gpu.double().to(DEV)
    pc = synthetic.make_batch(2000, B, N).double()
    target = torch.rand(B, N, generator=torch.Generator().manual_seed(1), dtype=torch.float64)
    return cpu, gpu, pc, target


def _same_geometry(a, b):
    assert [n for n, _ in a.log] == [n for n, _ in b.log] and len(a.log) == 9   # 3 FPS + 3 ball queries + 3 3-NN
    for (name, x), (_, y) in zip(a.log, b.log):
        assert torch.equal(x, y), name


def test_score_network_double_eval(nets):
    cpu, gpu, pc, _ = nets
    cpu.eval(); gpu.eval()
    ge, gk = _gpu_backend()
    ce, ck = _cpu_backend()
    with torch.no_grad():
        with backend(ge, gk):
            feat, score, _ = gpu(pc.to(DEV))
        with backend(ce, ck):
            feat_ref, score_ref, _ = cpu(pc)
    assert score.dtype == torch.float64 and feat.dtype == torch.float64
    _same_geometry(ge, ce)
    assert float((score.cpu() - score_ref).abs().max()) < 1e-10
    assert float((feat.cpu() - feat_ref).abs().max()) < 1e-9 * (1.0 + float(feat_ref.abs().max()))


def test_score_network_double_train_backward(nets):
    cpu, gpu, pc, target = nets
    cpu.train(); gpu.train()
    ge, gk = _gpu_backend()
    ce, ck = _cpu_backend()
    with backend(ge, gk):
        _, _, loss = gpu(pc.to(DEV), target.to(DEV))
        gpu.zero_grad()
        loss.backward()
    with backend(ce, ck):
        _, _, loss_ref = cpu(pc, target)
        cpu.zero_grad()
        loss_ref.backward()
    _same_geometry(ge, ce)
    assert abs(float(loss) - float(loss_ref)) <= 1e-10 * abs(float(loss_ref))
    named = dict(cpu.named_parameters())
    # gradients that vanish analytically (a bias in front of a train-mode BatchNorm) are rounding noise of differences of
    # large sums, ~1e-18 here: they are held to a floor of 1e-12 of the largest gradient instead of their own size
    floor = 1e-12 * max(float(p.grad.abs().max()) for p in named.values())
    bad = []
    for name, p in gpu.named_parameters():
        ref = named[name].grad
        assert p.grad is not None and p.grad.dtype == torch.float64, name
        err = float((p.grad.cpu() - ref).abs().max())
        if not err <= 1e-9 * float(ref.abs().max()) + floor:
            bad.append((name, err, float(ref.abs().max())))
    assert not bad, bad


def test_featureless_sa_block_double():
    from regnet_for_3d_grasping_amd.pn2_utils.modules import PointNetSAModule
    torch.manual_seed(3)
    sa = PointNetSAModule(in_channels=0, mlp_channels=(32, 64), num_centroids=256, radius=0.2, num_neighbours=64,
                          use_xyz=True).double().eval()
    sa_gpu = PointNetSAModule(in_channels=0, mlp_channels=(32, 64), num_centroids=256, radius=0.2, num_neighbours=64,
                              use_xyz=True)
    sa_gpu.load_state_dict(sa.state_dict())
    sa_gpu = sa_gpu.double().to(DEV).eval()
    xyz = torch.rand(2, 3, 2048, generator=torch.Generator().manual_seed(4), dtype=torch.float64)
    ge, gk = _gpu_backend()
    ce, ck = _cpu_backend()
    with torch.no_grad():
        with backend(ge, gk):
            new_xyz, feat = sa_gpu(xyz.to(DEV), None)       # the `feature is None` branch, on the operator path
        with backend(ce, ck):
            new_ref, feat_ref = sa(xyz, None)
    assert [n for n, _ in ge.log] == ["farthest_point_sample", "ball_query"]
    for (_, x), (_, y) in zip(ge.log, ce.log):
        assert torch.equal(x, y)
    assert torch.equal(new_xyz.cpu(), new_ref)
    assert float((feat.cpu() - feat_ref).abs().max()) < 1e-10 * (1.0 + float(feat_ref.abs().max()))


def test_float32_only_stages_refuse_float64():
    from regnet_for_3d_grasping_amd import pipeline
    from regnet_for_3d_grasping_amd.score_network import ScoreNetwork
    from regnet_for_3d_grasping_amd.train_step import ScoreTrainer
    net = ScoreNetwork(training=True).double().to(DEV).eval()
    pc = torch.rand(1, 1024, 6, dtype=torch.float64, device=DEV)
    for call in (lambda: net.plan(pc), lambda: net.sample_levels(pc), lambda: net.sample_level1(pc)):
        with pytest.raises(RuntimeError, match="float32 only"):
            call()
    score32, region32 = pipeline.build_models(DEV)
    with pytest.raises(RuntimeError, match="float32 only"):
        pipeline.forward_scenes(score32, region32, pc)
    pipe = pipeline.ForwardPipeline(score32, region32, with_region=False)
    with pytest.raises(RuntimeError, match="float32 only"):
        for _ in pipe.run([pc]):
            pass
    trainer = ScoreTrainer(net)
    with pytest.raises(RuntimeError, match="float32 only"):
        trainer.step(pc, torch.rand(1, 1024, dtype=torch.float64, device=DEV))
