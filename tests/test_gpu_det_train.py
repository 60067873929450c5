"""Deterministic mode, training level: under torch.use_deterministic_algorithms(True) two RefineTrainer runs from one
state_dict and the same torch / numpy seeds agree bit for bit -- every loss, gradient, parameter, BatchNorm running statistic
and num_batches_tracked -- eager, replayed (hipGraph), and eager against replayed; the mode's gradients stay as close to a
float64 evaluation as the default path's; toggling the flag re-captures the trainer's graphs."""
import numpy as np
import pytest
import torch

from tests.test_gpu_train_graphs import _batches, _named_grads, _trainer

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture
def det():
    was, warn = torch.are_deterministic_algorithms_enabled(), torch.is_deterministic_algorithms_warn_only_enabled()
    torch.use_deterministic_algorithms(True)
    try:
        yield
    finally:
        torch.use_deterministic_algorithms(was, warn_only=warn)


def _run(graphs, batches, iterations):
    """Adam at lr 1e-3, dropout on -> (losses, gradients, state of both networks, replays)."""
    torch.manual_seed(1234)
    t = _trainer(graphs, 1e-3, True)
    np.random.seed(7)
    losses = []
    for k in range(iterations):
        total, parts = t.step(*batches[k % len(batches)])
        losses.append(torch.stack([total.detach().float().reshape(())] +
                                  [v.detach().float().reshape(()) for _, v in sorted(parts.items()) if torch.is_tensor(v)]))
    torch.cuda.synchronize()
    state = {"score." + k: v.detach().clone() for k, v in t.score_net.state_dict().items()}
    state.update({"region." + k: v.detach().clone() for k, v in t.region_net.state_dict().items()})
    return [l.cpu() for l in losses], _named_grads(t), state, t.graph_replays


def _assert_bitwise(a, b):
    la, ga, sa, _ = a
    lb, gb, sb, _ = b
    for i, (x, y) in enumerate(zip(la, lb)):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32)), ("losses", i, x, y)
    assert ga.keys() == gb.keys()
    for k in ga:
        assert (ga[k] is None) == (gb[k] is None), k
        if ga[k] is not None:
            assert torch.equal(ga[k].view(torch.int32), gb[k].view(torch.int32)), ("gradient", k)
    assert sa.keys() == sb.keys()
    for k in sa:
        x, y = sa[k], sb[k]
        if x.is_floating_point():
            x, y = x.view(torch.int32), y.view(torch.int32)
        assert torch.equal(x, y), ("state", k)


def test_two_eager_runs_agree_bitwise(det):
    batches = _batches(2, 2, 6144, 8300)
    a = _run(False, batches, 6)
    b = _run(False, batches, 6)
    _assert_bitwise(a, b)
    assert any(k.endswith("num_batches_tracked") and int(v) == 6 for k, v in a[2].items())


def test_replayed_runs_agree_bitwise_with_each_other_and_with_eager(det):
    batches = _batches(2, 2, 6144, 8300)
    eager = _run(False, batches, 6)
    g1 = _run(True, batches, 6)
    g2 = _run(True, batches, 6)
    assert g1[3] == g2[3] == 4
    _assert_bitwise(g1, g2)
    _assert_bitwise(eager, g1)      # test_gpu_train_graphs.py can only ask for an envelope here without the mode


def test_config3_runs_agree_bitwise(det):
    batches = _batches(1, 8, 25600, 9100)
    a = _run(False, batches, 3)
    b = _run(False, batches, 3)
    _assert_bitwise(a, b)


def test_gradients_against_fp64(det):
    """The mode changes the order of the additions, not the accuracy: the yardstick of test_gpu_train.py."""
    from regnet_for_3d_grasping_amd import synthetic
    from regnet_for_3d_grasping_amd.score_network import ScoreNetwork
    from tests.test_gpu_train import _check_gradients_against_fp64
    B, N = 2, 6144
    pc = synthetic.make_batch(8400, B, N).to(DEV)
    target = torch.from_numpy(np.random.default_rng(6).uniform(0, 1, (B, N)).astype(np.float32)).to(DEV)
    gpu = ScoreNetwork(training=True)
    gpu.load_state_dict(synthetic.seeded_state_dict(gpu, 3))
    gpu = gpu.to(DEV).train()
    gpu.extrat_featurePN2.mlp.dropout_prob = 0.0
    _, _, loss = gpu(pc, target)
    loss.backward()
    assert torch.isfinite(loss)
    native, _ = _check_gradients_against_fp64(gpu, pc, target)
    assert len(native) >= 60


def test_toggling_the_flag_recaptures():
    was, warn = torch.are_deterministic_algorithms_enabled(), torch.is_deterministic_algorithms_warn_only_enabled()
    try:
        torch.use_deterministic_algorithms(False)
        t = _trainer(True, 0.0, False)
        small = _batches(1, 2, 6144, 8500)[0]
        np.random.seed(3)
        for _ in range(3):
            t.step(*small)
        assert t.graph_replays == 1 and t._graphs is not None and t._graphs.signature[-1] is False
        torch.use_deterministic_algorithms(True)
        t.step(*small)                  # the captured kernels are the default ones: eager, then a new capture
        assert t.graph_replays == 1 and t._graphs is None
        for _ in range(3):
            t.step(*small)
        assert t.graph_replays > 1 and t._graphs is not None and t._graphs.signature[-1] is True
    finally:
        torch.use_deterministic_algorithms(was, warn_only=warn)
