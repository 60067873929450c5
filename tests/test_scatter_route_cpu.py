"""The case table of the gather / scatter tests (tests/scatter_cases.py) against ``regnet_scatter_segsum_route`` and
``regnet_scatter_atomic_route``, the host functions the launchers of the group_points / gather_knn / interpolate backwards take
their kernel from: every row takes the route it names in all three modes, and the table as a whole reaches every route, every
channels-per-workgroup value the halving can give, both sides of every path boundary and the plan kernels' edges.  No GPU."""
import ctypes

import numpy as np
import pytest

from . import scatter_cases as cases

OK, ERR_SHAPE, ERR_NULL, ERR_UNSUPPORTED = cases.OK, cases.ERR_SHAPE, cases.ERR_NULL, cases.ERR_UNSUPPORTED


@pytest.mark.parametrize("case", cases.CASES, ids=[c.id for c in cases.CASES])
def test_row_takes_the_routes_it_names(case):
    r = cases.routes(case)
    assert r["seg32"][:2] == case.seg32 and r["seg64"][:2] == case.seg64 and r["atomic"] == case.atomic, r
    for name in ("seg32", "seg64"):
        kind, cpb, chunk = r[name]
        assert (kind == "chunks") == (0 < chunk < cases.num_slots(case)), (name, r[name])
        assert (kind == "one") == (chunk == cases.num_slots(case)), (name, r[name])
    # tensors stay small: the float64 gradient and output of a row
    assert 8 * case.B * case.C * (cases.num_slots(case) + case.R) <= 160e6
    if case.op == "knn":
        assert case.R == case.rows


@pytest.mark.parametrize("case", cases.CASES, ids=[c.id for c in cases.CASES])
def test_index_table_of_a_row_carries_every_edge(case):
    idx = cases.index(case).numpy().reshape(case.B, -1)
    R, L = case.R, cases.num_src(case)
    assert idx.shape == (case.B, L) and np.array_equal(idx, cases.index(case).numpy().reshape(case.B, -1))
    per_slot = 3 if cases.weighted(case) else 1
    for b in range(case.B):
        row = idx[b]
        ok = (row >= 0) & (row < R)
        assert set(cases.bad_values(R)) <= set(row[~ok].tolist())
        count = np.bincount(row[ok], minlength=R)
        assert all(count[n] > 0 for n in cases.required(case)) and all(count[e] == 0 for e in cases.empties(case))
        assert count[0] > 0 and count[R - 1] > 0
        assert all(count[n] > 0 for n in range(R) if n % 1024 in (0, 1023) and n not in cases.empties(case))
        if L >= 192:
            steps = row[:L // 64 * 64].reshape(-1, 64)
            assert any(len(set(s.tolist())) == 1 and 0 <= s[0] < R for s in steps)
            if R >= 64:
                assert any(len(set(s.tolist())) == 64 and s.min() >= 0 and s.max() < R for s in steps)
        edges = cases.chunk_edges(case)
        for e in edges:
            # one destination's segment continues across the edge, and destination 0 has a source in the chunk before it
            run = row[(e - 1) * per_slot:(e + 1) * per_slot]
            assert len(set(run.tolist())) == 1 and 0 <= run[0] < R
        for lo, hi in zip([0] + edges, edges + [cases.num_slots(case)]):
            if edges and hi - lo >= 4094:
                assert (row[lo * per_slot:hi * per_slot] == 0).any(), (lo, hi)
    # the exact inputs are exact (asserted by the generator) and the same on every call
    g, w = cases.exact_inputs(case, cases.index(case))
    assert float(g.abs().max()) <= 1024 and bool((g == g.round()).all())
    assert w is None or set(np.unique(w.numpy()).tolist()) <= {0.0, 0.25, 0.5, 1.0}


def _all(name):
    return [(c, cases.routes(c)[name]) for c in cases.CASES]


def test_table_reaches_every_route_and_every_channel_count():
    for name in ("seg32", "seg64"):
        for is_weighted in (False, True):
            rows = [(c, r) for c, r in _all(name) if cases.weighted(c) == is_weighted]
            assert {r[0] for _, r in rows} == {"one", "chunks", "global"}, (name, is_weighted)
            # the global kernel with a last, partial channel block
            assert any(r[0] == "global" and c.C % r[1] for c, r in rows), (name, is_weighted)
        one = [(c, r) for c, r in _all(name) if r[0] == "one"]
        assert {r[1] for _, r in one} >= {1, 2, 3, 4, 7, 8}, name
        for cpb in (2, 3, 4, 7, 8):     # ... each with a last workgroup that holds fewer channels
            assert any(r[1] == cpb and c.C % cpb for c, r in one), (name, cpb)
        assert all(r[1] == 1 for _, r in _all(name) if r[0] == "chunks")
        # both kernels of the family take several channels per workgroup
        assert any(r[1] > 1 and cases.weighted(c) for c, r in one) and any(r[1] > 1 and not cases.weighted(c) for c, r in one)
    for is_weighted in (False, True):
        rows = [(c, r) for c, r in _all("atomic") if cases.weighted(c) == is_weighted]
        assert {r[0] for _, r in rows} == {"lds", "global"}, is_weighted
        assert any(r[0] == "global" and c.C % r[1] for c, r in rows), is_weighted
        assert any(r[0] == "lds" and r[1] == 32 and c.C % 32 for c, r in rows), is_weighted
    lds = [(c, r) for c, r in _all("atomic") if r[0] == "lds"]
    assert {r[1] for _, r in lds} >= {1, 2, 4, 8, 16, 32}
    for cpb in (2, 4, 8, 16, 32):
        assert any(r[1] == cpb and c.C % cpb for c, r in lds), cpb
    assert {c.op for c in cases.CASES} == {"group", "knn", "interp"}
    assert len({c.id for c in cases.CASES}) == len(cases.CASES)


def _has(name, is_weighted, kind, **want):
    for c, r in _all(name):
        have = {"slots": cases.num_slots(c), "R": c.R, "chunk": r[2] if len(r) > 2 else None}
        if cases.weighted(c) == is_weighted and r[0] == kind and all(have[k] == v for k, v in want.items()):
            return True
    return False


def test_table_has_a_row_on_each_side_of_every_path_boundary():
    for is_weighted in (False, True):
        # one chunk | several chunks, in slots
        assert _has("seg32", is_weighted, "one", slots=36864) and _has("seg32", is_weighted, "chunks", slots=36865)
        assert _has("seg64", is_weighted, "one", slots=18432) and _has("seg64", is_weighted, "chunks", slots=18433)
        # several chunks | global kernel, in destinations (the last chunked layout stages 4096 slots)
        assert _has("seg32", is_weighted, "chunks", R=16384, chunk=4096) and _has("seg32", is_weighted, "global", R=16385)
        assert _has("seg64", is_weighted, "chunks", R=9557, chunk=4096) and _has("seg64", is_weighted, "global", R=9558)
        # LDS atomics | global atomics, in destinations
        assert _has("atomic", is_weighted, "lds", R=36864) and _has("atomic", is_weighted, "global", R=36865)
    # the unweighted slot counts as products rows x K
    shapes = {(c.rows, c.K) for c in cases.CASES if c.op == "group"}
    assert {(36865, 1), (7373, 5), (577, 64)} <= shapes
    # one layout of 4094 slots would be the next: it is the global kernel's
    assert cases.segsum_route(4, 0, 2, 3, 16385, 36865)[1] == ("global", 4, 0)


def test_table_has_the_plan_edges():
    plan = [c for c in cases.CASES if "plan" in c.tags]
    assert {c.R for c in plan} >= {1, 2, 63, 64, 65, 1023, 1024, 1025, 2049}
    assert {cases.num_src(c) % 64 for c in plan} >= {0, 1, 63}
    for op in ("group", "interp"):
        assert {c.R for c in plan if c.op == op} & {1, 2} and {c.R for c in plan if c.op == op} & {2049}


def test_routes_return_the_launchers_error_codes():
    seg, atom = cases.segsum_route, cases.atomic_route
    none3, none2 = (None, 0, 0), (None, 0)
    assert seg(2, 0, 1, 1, 1, 1) == (ERR_SHAPE, none3) and seg(4, 1, 1, 1, 1, 4) == (ERR_SHAPE, none3)
    assert seg(4, 0, -1, 1, 1, 1) == (ERR_SHAPE, none3) and atom(1, 1, -1, 1) == (ERR_SHAPE, none2)
    for empty in ((0, 1, 1, 1), (1, 0, 1, 1), (1, 1, 0, 1), (1, 1, 1, 0)):
        assert seg(4, 0, *empty) == (OK, none3) and atom(*empty) == (OK, none2)
        assert seg(8, 1, *empty[:3], 3 * empty[3]) == (OK, none3)
    # more scenes than a grid dimension holds: what the plan, the segment sums and both atomic launchers answer
    assert seg(4, 0, 65536, 1, 1, 1) == (ERR_UNSUPPORTED, none3) and seg(8, 1, 65536, 1, 1, 3) == (ERR_UNSUPPORTED, none3)
    assert atom(65536, 1, 1, 1) == (ERR_UNSUPPORTED, none2) and atom(65535, 1, 1, 1) == (OK, ("lds", 32))
    # channel blocks beyond grid.y: 4 per thread in float32, 8 in float64, 16 per block of the atomic kernels
    assert seg(4, 0, 1, 4 * 65535, 16385, 36865)[0] == OK and seg(4, 0, 1, 4 * 65535 + 1, 16385, 36865)[0] == ERR_UNSUPPORTED
    assert seg(8, 0, 1, 8 * 65535, 9558, 18433)[0] == OK and seg(8, 0, 1, 8 * 65535 + 1, 9558, 18433)[0] == ERR_UNSUPPORTED
    assert seg(8, 0, 1, 8 * 65535 + 1, 40, 60)[0] == ERR_UNSUPPORTED     # the float64 entry points refuse these whatever the route
    assert atom(1, 16 * 65535, 36865, 1)[0] == OK and atom(1, 16 * 65535 + 1, 36865, 1)[0] == ERR_UNSUPPORTED
    assert atom(1, 2 ** 31 - 1, 36864, 1)[1][0] == "lds" and atom(1, 2 ** 31, 36864, 1)[0] == ERR_UNSUPPORTED
    assert seg(4, 0, 1, 1, 2 ** 30, 1)[0] == ERR_UNSUPPORTED and seg(4, 0, 1, 1, 1, 2 ** 31)[0] == ERR_UNSUPPORTED
    from regnet_for_3d_grasping_amd import _lib
    assert _lib.call("regnet_scatter_segsum_route", None, 4, 0, 1, 1, 1, 1, None) == ERR_NULL
    assert _lib.call("regnet_scatter_atomic_route", None, 1, 1, 1, 1, None) == ERR_NULL


def test_routes_need_no_device_pointer():
    """Host memory in, host memory out: the three (two) words are all the functions touch."""
    from regnet_for_3d_grasping_amd import _lib
    buf = (ctypes.c_int64 * 5)(*([-5] * 5))
    assert _lib.call("regnet_scatter_segsum_route", None, 8, 1, 2, 3, 50, 3 * 18433, ctypes.addressof(buf) + 8) == OK
    assert list(buf) == [-5, 2, 1, 18357, -5]
    buf = (ctypes.c_int64 * 4)(*([-5] * 4))
    assert _lib.call("regnet_scatter_atomic_route", None, 16, 1023, 40, 60, ctypes.addressof(buf) + 8) == OK
    assert list(buf) == [-5, 1, 32, -5]


def test_summation_bound_is_the_any_order_bound():
    import torch
    n, S = torch.tensor([0.0, 1.0, 3.0, 300.0]), torch.tensor([0.0, 2.0, 5.0, 1e4])
    u = 2.0 ** -24
    want = [0.0, 2 * u * 2 / (1 - 2 * u), 4 * u * 5 / (1 - 4 * u), 301 * u * 1e4 / (1 - 301 * u)]
    assert cases.summation_bound(n.double(), S.double()).tolist() == pytest.approx(want, rel=1e-14)
    # through the references: one destination with two contributions, one with none
    g = torch.tensor([[[[3.0, -4.0]]]])
    idx = torch.tensor([[[1, 1]]])
    assert cases.group_bound(g, idx, 2)[0, 0].tolist() == pytest.approx([0.0, 3 * u * 7 / (1 - 3 * u)], rel=1e-14)
    w = torch.tensor([[[0.5, 0.25, 1.0]]])
    b = cases.interpolate_bound(torch.tensor([[[8.0]]]), torch.tensor([[[0, 0, 5]]]), w, 2)[0, 0].tolist()
    assert b == pytest.approx([3 * u * 6 / (1 - 3 * u), 0.0], rel=1e-14)


def test_references_refuse_an_index_of_another_row_count():
    import torch
    from . import det_reference as D, f64_reference as F
    for ref, dt in ((F, torch.float64), (D, torch.float32)):
        g, w = torch.zeros(1, 2, 5, dtype=dt), torch.zeros(1, 5, 3, dtype=dt)
        with pytest.raises(RuntimeError, match="shape mismatch"):
            ref.interpolate_backward(g, torch.zeros(1, 4, 3, dtype=torch.int64), w, 7)
        with pytest.raises(RuntimeError, match="shape mismatch"):
            ref.interpolate_backward(g, torch.zeros(1, 6, 3, dtype=torch.int64), w, 7)
        assert tuple(ref.interpolate_backward(g, torch.zeros(1, 5, 3, dtype=torch.int64), w, 7).shape) == (1, 2, 7)
