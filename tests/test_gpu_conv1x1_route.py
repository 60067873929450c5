"""The training 1x1 convolutions launch what the case table (tests/conv1x1_cases.py) says: for every row a real forward +
backward with the library's entry points recorded, and the statistics a convolution leaves for the BatchNorm behind it
(``_bn_sums``: an uninitialised buffer unless the forward filled it) present exactly where the row says, and right."""
import pytest
import torch

from . import conv1x1_cases as cases

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FIRST = 48          # input channels of the stack in front of a pending row's convolution: no row has (Co, Ci) = (Ci, 48)


@pytest.fixture
def recorded(monkeypatch):
    """[(entry point, Co, Ci)] of every launch of a ``regnet_conv1x1_*`` entry point from here on."""
    from regnet_for_3d_grasping_amd import _lib
    calls, call = [], _lib.call

    def recording(name, anchor, *args, **kwargs):
        if name.startswith("regnet_conv1x1_") and _lib.HAS_STREAM[name]:
            params = _lib.PARAMS[name]
            calls.append((name, args[params.index("Co")], args[params.index("Ci")]))
        return call(name, anchor, *args, **kwargs)
    monkeypatch.setattr(_lib, "call", recording)
    return calls


def _input(B, C, L, aligned=True):
    if aligned:
        return torch.randn(B, C, L, device=DEV, requires_grad=True)
    x = torch.randn(B * C * L + 1, device=DEV)[1:].view(B, C, L).requires_grad_(True)      # starts 4 bytes into a 16-byte line
    assert x.data_ptr() % 16 == 4 and x.is_contiguous()
    return x


def _of_layer(calls, Co, Ci, pad):
    return [name for name, co, ci in calls if (co, ci) == (Co, pad or Ci)]


def _check_sums(y, stats):
    """``y._bn_sums`` is there iff ``stats``, and then holds the per-channel sum / sum of squares of y: against the float64 sums
    of y itself the error is the summation's alone (the bounds of test_statistics_left_by_the_convolution)."""
    sums = getattr(y, "_bn_sums", None)
    assert (sums is not None) == stats
    if sums is None:
        return
    y = y.detach().flatten(2).double()
    n = y.shape[0] * y.shape[2]
    s_own, q_own = y.sum((0, 2)), (y * y).sum((0, 2))
    err_s = float(((sums[0::2] - s_own).abs() / (q_own * n).sqrt()).max())
    err_q = float(((sums[1::2] - q_own).abs() / q_own).max())
    print("sums: sum %.3e, sum of squares %.3e (bound 2e-7)" % (err_s, err_q))
    assert err_s < 2e-7 and err_q < 2e-7


def _run(case, recorded, monkeypatch, between=None):
    """Forward + backward of the row's convolution under its switches (``between``: called after the forward); returns the
    launches of that convolution."""
    from regnet_for_3d_grasping_amd.pn2_utils.nn import SharedMLP
    B, Co, Ci, L = case.shape
    route = case.expect if case.expect is not None else case.otherwise
    torch.manual_seed(Co + Ci + L)
    with cases.switched(case.switches) as c:
        if case.kind == "plain":
            conv = torch.nn.Conv1d(Ci, Co, 1, bias=False).to(DEV)
            x = _input(B, Ci, L, case.switches.get("aligned", True))
            assert c.supported(conv, x)
            y = c.conv1x1(conv, x, stats=True)
            out = y
        else:
            outputs = []

            def keeping(fn):      # the blocks call both through the module: keep what they return
                def kept(*args, **kwargs):
                    outputs.append(fn(*args, **kwargs))
                    return outputs[-1]
                return kept
            monkeypatch.setattr(c, "conv1x1", keeping(c.conv1x1))
            monkeypatch.setattr(c, "conv1x1_of_pending", keeping(c.conv1x1_of_pending))
            mlp = SharedMLP(FIRST, (Ci, Co), ndim=1).to(DEV).train()
            x = _input(B, FIRST, L)
            before = c.DEFERRED["layers"]
            out = mlp(x)
            assert c.DEFERRED["layers"] - before == (case.expect is not None)
            assert len(outputs) == 2
            y = outputs[1]
        assert y.shape == (B, Co, L)
        _check_sums(y, route[2])
        if between is not None:
            between(c)
        out.backward(torch.randn_like(out))
        assert x.grad is not None and bool(torch.isfinite(x.grad).all())
    return _of_layer(recorded, Co, Ci, route[1])


@pytest.mark.parametrize("case", cases.CASES, ids=cases.case_id)
def test_a_layer_launches_what_its_row_says(case, recorded, monkeypatch):
    assert _run(case, recorded, monkeypatch) == cases.launches(case)


@pytest.mark.parametrize("kind", ["plain", "pending"])
def test_the_backward_takes_the_forwards_route(kind, recorded, monkeypatch):
    """The route is chosen once, before the forward, and kept with the autograd node: a switch that moves between forward and
    backward does not move the layer's backward onto other kernels."""
    case = next(c for c in cases.CASES if c.kind == kind and c.shape == (2, 64, 64, 256) and not c.switches)

    def flip(c):
        assert c.STREAM
        c.STREAM = False
    try:
        assert _run(case, recorded, monkeypatch, between=flip) == cases.launches(case)
    finally:
        from regnet_for_3d_grasping_amd import conv1x1_train
        conv1x1_train.STREAM = True
