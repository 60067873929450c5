"""``fused.sa_route`` / ``fused.fp_route`` against the hand-written table (tests/fused_cases.py), and their invariants over a
sweep of widths around every threshold under every single-switch override.  No GPU: the routes read shapes and flags of a
module -- a CPU module or a stand-in -- and plain integers."""
import itertools

import pytest

from . import fused_cases as cases

OVERRIDES = [{}] + [{k: False} for k in cases.SWITCHES]
around = lambda values: sorted({v + d for v in values for d in (-1, 0, 1) if v + d >= 0})


@pytest.mark.parametrize("case", cases.SA_CASES, ids=cases.case_id)
def test_every_set_abstraction_row_takes_the_route_written_beside_it(case):
    with cases.switched(case) as fused:
        got = fused.sa_route(cases.sa_stand_in(case), case.has_feature)
        assert (None if got is None else tuple(got)) == case.expect
        real = cases.sa_module(case)
        assert real is not None or case.relu is not None
        if real is not None:            # a row is right only if the real module of its description takes the same route
            assert fused.sa_route(real, case.has_feature) == got


@pytest.mark.parametrize("case", cases.FP_CASES, ids=cases.case_id)
def test_every_feature_propagation_row_takes_the_route_written_beside_it(case):
    def route(module, seg):
        return fused.fp_route(module, case.Cs, case.Cd, case.Ns, case.Nd, seg=seg, f32=case.f32)
    with cases.switched(case) as fused:
        got = route(*cases.fp_stand_in(case))
        assert (None if got is None else tuple(got)) == case.expect
        assert (got is None) <= (case.seg is not None)
        real = cases.fp_module(case)
        if real is not None:
            assert route(*real) == got


def test_the_table_reaches_every_value_of_every_field():
    for rows, fields, values in ((cases.SA_CASES, cases.SA_FIELDS, cases.SA_VALUES), (cases.FP_CASES, cases.FP_FIELDS, cases.FP_VALUES)):
        routes = [case.expect for case in rows if case.expect is not None]
        for i, field in enumerate(fields):
            assert {r[i] for r in routes} == values[field], field
        assert any(case.expect is None for case in rows)
        assert any(not case.switches for case in rows)                                     # every switch on ...
        assert set().union(*(case.switches for case in rows)) == set(cases.SWITCHES)      # ... and each one off
        assert {v for case in rows for v in case.switches.values()} == {False}
    # the reference network, default switches: its three set-abstraction and three feature-propagation blocks, the last with ``seg``
    from regnet_for_3d_grasping_amd import pointnet2
    ins = (3,) + tuple(c[-1] for c in pointnet2._SA_CHANNELS)
    want = {(Cf, widths) for Cf, widths in zip(ins, pointnet2._SA_CHANNELS)}
    assert want <= {(c.Cf, c.widths) for c in cases.SA_CASES if not c.switches and c.mode == "eval" and c.relu is None}
    sparse, fps = ins[-1], set()
    for level, widths in enumerate(pointnet2._FP_CHANNELS):
        fps.add((sparse, ins[-2 - level], widths, level == len(pointnet2._FP_CHANNELS) - 1))
        sparse = widths[-1]
    assert fps <= {(c.Cs, c.Cd, c.widths, c.seg == 1) for c in cases.FP_CASES if not c.switches}


@pytest.mark.parametrize("switches", OVERRIDES, ids=lambda s: "-".join("%s=%d" % kv for kv in s.items()) or "default")
def test_set_abstraction_invariants_around_every_threshold(switches):
    firsts, seconds, lasts = around([40, 64, 128, 256, 512]), [128, 256, 512], around([256, 512, 1024])
    for (Cf, has_feature), first, second, last, n, relu1 in itertools.product(
            [(0, False), (3, True), (5, True), (6, True), (128, True)], firsts, seconds, lasts, (2, 3, 4), (True, False)):
        widths = ((first, last), (first, second, last), (first, second, second, last))[n - 2]
        relu = (relu1,) + (True,) * (n - 1)
        routes = {}
        for mode in ("eval", "train", "grad"):
            case = cases._sa(Cf, widths, None, relu=relu, has_feature=has_feature, mode=mode, **switches)
            with cases.switched(case) as fused:
                routes[mode] = r = fused.sa_route(cases.sa_stand_in(case), has_feature)
            what = (case, r)
            for field, value in zip(cases.SA_FIELDS, r):
                assert value in cases.SA_VALUES[field] or (field == "tail" and value == 3), what
            # the kernel named pools itself, or exactly the layers it leaves follow it
            assert r.tail == n - {"layer1": 1, "layer12": 2, "premul_layer": 2}.get(r.features, n), what
            # the geometry stage prepares what the route's kernels read, and nothing that nobody reads
            assert (r.prepare == "pairs") == (r.features == "chain3"), what
            assert (r.prepare == "premul") == (r.features.startswith("premul") and mode == "eval"), what
            assert not (r.features.startswith("premul") and not has_feature), what
        # the mode decides what is prepared ahead, never which kernels run; in training mode or under autograd nothing is
        # prepared that reads a weight: at most the pairing, and only where the geometry stage has always made it (a 3-layer
        # block of at most 8 input channels)
        assert len({r.features for r in routes.values()}) == len({r.tail for r in routes.values()}) == 1, routes
        always = "pairs" if switches.get("CHAIN3", True) and n == 3 and Cf + 3 <= 8 else None
        assert all(routes[mode].prepare in (None, always) for mode in ("train", "grad")), routes


@pytest.mark.parametrize("switches", OVERRIDES, ids=lambda s: "-".join("%s=%d" % kv for kv in s.items()) or "default")
def test_feature_propagation_invariants_around_every_threshold(switches):
    for Cs, Cd, first, seg, f32 in itertools.product(around([256, 512]), around([0, 4, 8, 64]), around([96, 256, 1024, 2048]),
                                                     (None, 1, 2), (True, False)):
        widths = (first, 256, 256)
        base = cases._fp(Cs, Cd, widths, None, Ns=None, Nd=None, seg=seg, f32=f32, **switches)
        with cases.switched(base) as fused:
            def route(Ns, Nd, seg=seg):
                module, net = cases.fp_stand_in(base._replace(seg=seg))
                return fused.fp_route(module, Cs, Cd, Ns, Nd, seg=net, f32=f32)
            r = route(None, None)
            what = (base, r)
            # a caller that knows widths only (prepack) is answered as one with fewer sparse points than dense ones
            assert r == route(16, 129) == route(5120, 25600), what
            assert route(129, 129) in (None, fused.FpRoute("concat", None)) and route(200, 129) == route(129, 129), what
            alone = route(None, None, seg=None)
            assert alone is not None and alone.features in ("premul", "concat"), what
            if r is None:
                assert seg is not None, what
                continue
            for field, value in zip(cases.FP_FIELDS, r):
                assert value in cases.FP_VALUES[field], what
            assert r.features.startswith("head") == (seg is not None), what
            # block + head as one kernel starts from the pre-multiplied first layer, with the same skip input
            assert not r.features.startswith("head") or (alone.features == "premul" and alone.skip == r.skip and seg == 1), what
            assert (r.skip is None) == (r.features == "concat" or Cd == 0), what
            assert r.features != "head_interp" or (r.skip != "gemm" and switches.get("FP_HEAD_INTERP", True)), what
            assert r.features == "concat" or (f32 and switches.get("PREMUL", True) and Cs % 4 == 0), what
