"""``conv1x1_train.route`` against the hand-written table (tests/conv1x1_cases.py), and its invariants over a sweep of every
threshold of the shape predicates under every single-switch override.  No GPU: the route takes integers and bools, and the
predicates it asks are host code of the library."""
import itertools
import types

import pytest
import torch

from . import conv1x1_cases as cases

CI = [8, 9, 31, 32, 33, 48, 256, 259, 272, 512, 515, 528, 1024]
CO = [3, 16, 32, 40, 256, 272]
LS = [60, 64, 77, 256, 1000, 4160]
OVERRIDES = [{}] + [{k: k == "SPLIT_PRODUCTS"} for k in cases.SWITCHES] + [{"deterministic": True}, {"aligned": False}]


def _route(c, case_or_shape, switches, affine, want_stats=True):
    return c.route(*case_or_shape, aligned=switches.get("aligned", True), affine=affine, want_stats=want_stats)


@pytest.mark.parametrize("case", cases.CASES, ids=cases.case_id)
def test_every_row_takes_the_route_written_beside_it(case):
    with cases.switched(case.switches) as c:
        got = _route(c, case.shape, case.switches, case.kind == "pending")
        assert (None if got is None else tuple(got)) == case.expect
        if case.kind == "pending":
            assert (case.otherwise is None) == (case.expect is not None)
        if case.otherwise is not None:
            assert tuple(_route(c, case.shape, case.switches, False)) == case.otherwise
        # without a BatchNorm behind the layer: the same kernels, no statistics
        bare = _route(c, case.shape, case.switches, case.kind == "pending", want_stats=False)
        assert (None if bare is None else tuple(bare)) == (case.expect and case.expect[:2] + (False,) + case.expect[3:])


def test_the_table_reaches_every_value_of_every_field():
    routes = [r for case in cases.CASES for r in (case.expect, case.otherwise) if r is not None]
    for i, field in enumerate(cases.FIELDS):
        seen = {bool(r[i]) if field == "pad" else r[i] for r in routes}
        assert seen == cases.VALUES[field], field
    assert any(case.expect is None for case in cases.CASES)
    overridden = set().union(*(case.switches for case in cases.CASES))
    assert overridden == set(cases.SWITCHES) | {"deterministic", "aligned"}
    assert {case.switches.get(k) for case in cases.CASES for k in cases.SWITCHES if k in case.switches} == {False, True}


def _conv(Co, Ci):
    """What ``supported`` / ``pending_ok`` read of a bias-free kernel-size-1 Conv1d, without its weights."""
    return types.SimpleNamespace(kernel_size=(1,), stride=(1,), dilation=(1,), padding=(0,), groups=1, bias=None,
                                 weight=types.SimpleNamespace(shape=(Co, Ci, 1)))


def _activation(B, Ci, L):
    """... and of a float32 activation on the GPU."""
    return types.SimpleNamespace(is_cuda=True, dtype=torch.float32, shape=(B, Ci, L), dim=lambda: 3, numel=lambda: B * Ci * L)


@pytest.mark.parametrize("switches", OVERRIDES, ids=lambda s: "-".join("%s=%d" % kv for kv in s.items()) or "default")
def test_invariants_around_every_threshold(switches):
    around = lambda values: sorted({v + d for v in values for d in (-1, 0, 1)})
    with cases.switched(switches) as c:
        for Co, Ci, L in itertools.product(around(CO), around(CI), around(LS)):
            for affine in (False, True):
                r = _route(c, (2, Co, Ci, L), switches, affine)
                what = (Co, Ci, L, affine, r)
                assert (r is None) <= affine, what
                assert c.pending_ok(_conv(Co, Ci), _activation(2, Ci, L)) == (_route(c, (2, Co, Ci, L), {}, True) is not None), what
                if r is None:
                    assert not c.stats_ok(Co, Ci, L, affine), what
                    continue
                for field, value in zip(cases.FIELDS, r):
                    assert (bool(value) if field == "pad" else value) in cases.VALUES[field], what
                # sums is an uninitialised buffer the next BatchNorm trusts: only a forward that fills it may promise it
                assert not r.stats or r.fwd in ("stream", "smallci"), what
                assert (r.fwd == "split") == (r.dgrad == "split"), what
                assert not r.pad or (r.pad > Ci and r.fwd in ("stream", "tile", "split") and r.wgrad == "tgemm"), what
                assert (r.fwd == "bmm") <= (r.dgrad == "bmm" and r.wgrad == "bmm"), what
                assert (r.wgrad == "smallci") == (r.fwd == "smallci"), what
                # stats_ok speaks of native_fwd / native_fwd_bnrelu on the shape as it is
                assert c.stats_ok(Co, Ci, L, affine) == bool(r.stats and r.fwd == "stream" and not r.pad), what


def test_padding_is_never_more_than_the_layer():
    """The rule ``max(32, ceil16(Ci))`` gives 32 or at most Ci + 15, so "not worth it" (more than 2 Ci + 32) cannot happen from
    9 channels up."""
    assert all(max(32, (Ci + 15) // 16 * 16) <= 2 * Ci + 32 for Ci in range(9, 4097))
