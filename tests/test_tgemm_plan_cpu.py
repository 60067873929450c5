"""The case table of the training-GEMM tests (tests/tgemm_cases.py) against the host side of csrc/tgemm.hip: the support predicates,
the weight gradient's slice rule and its workspace size give what every row expects by hand, and the table as a whole reaches
every kernel instantiation the launchers can start and both sides of every limit.  No GPU."""
import pytest

from . import tgemm_cases as cases

IDS = [c.id for c in cases.CASES]


def q(name, *args):
    from regnet_for_3d_grasping_amd import _lib
    assert not _lib.HAS_STREAM[name], name     # a host-side query: nothing is launched
    return int(_lib.call(name, None, *args))


def test_ids_are_unique_and_rejections_name_rows():
    assert len(set(IDS)) == len(IDS)
    assert len({r.id for r in cases.REJECTS}) == len(cases.REJECTS)
    for r in cases.REJECTS:
        assert r.base in cases.BY_ID, r
        assert set(r.override) <= {"B", "Co", "Ci", "L"}, r
        assert bool(r.override) != bool(r.fault), r       # one reason per refusal


@pytest.mark.parametrize("case", cases.GEMM_CASES, ids=[c.id for c in cases.GEMM_CASES])
def test_gemm_row_is_supported_as_the_row_says(case):
    assert case.op in ("fwd", "dgrad", "wgrad") and case.B >= 1 and case.why
    assert case.relu in (0, 1) and (case.affine or not case.relu)
    assert q("regnet_conv1x1_train_supported", case.Co, case.Ci, case.L) == 1
    if case.op == "dgrad":
        assert not case.affine and not case.stats
    if case.op == "fwd":
        if case.affine:
            assert q("regnet_conv1x1_bnrelu_supported", case.Co, case.Ci, case.L) == 1
        if case.stats:
            assert q("regnet_conv1x1_fwd_stats_supported", case.Co, case.Ci, case.L, case.affine) == 1
        assert case.slices is None and case.tile_n is None and case.workspace is None
    # buffers stay small enough for a case to take seconds
    assert case.B * max(case.Co, case.Ci) * case.L * 4 <= 64e6


@pytest.mark.parametrize("case", [c for c in cases.GEMM_CASES if c.op == "wgrad"], ids=[c.id for c in cases.GEMM_CASES if c.op == "wgrad"])
def test_weight_gradient_row_gets_its_slices_and_workspace(case):
    assert not case.stats and case.L % 16 == 0
    if case.affine:
        assert q("regnet_conv1x1_bnrelu_supported", case.Co, case.Ci, case.L) == 1
    S = q("regnet_conv1x1_wgrad_slices", case.B, case.Co, case.Ci, case.L)
    assert S == case.slices, (case.id, S)
    n = case.B * case.slices
    assert case.workspace == (n > 1)
    nbytes = q("regnet_conv1x1_wgrad_workspace_bytes", case.B, case.Co, case.Ci, case.L)
    assert nbytes == (n * case.Co * case.Ci * 4 if case.workspace else 0), (case.id, nbytes)
    assert case.tile_n == (128 if case.Ci <= 128 else 256)
    # a slice is whole, a multiple of 16 and at least two k-tiles deep (the kernel's prologue issues two)
    assert case.L % case.slices == 0 and (case.L // case.slices) % 16 == 0 and case.L // case.slices >= 32


@pytest.mark.parametrize("name,args,want", cases.LIMITS, ids=["%s%r" % (n[len("regnet_conv1x1_"):], a) for n, a, _ in cases.LIMITS])
def test_both_sides_of_every_limit(name, args, want):
    assert q(name, *args) == want


def test_limits_list_has_both_sides_of_each_limit():
    have = {(n[len("regnet_conv1x1_"):], a): w for n, a, w in cases.LIMITS}
    t, b, s = "train_supported", "bnrelu_supported", "fwd_stats_supported"
    for accepted, refused in [((t, (32, 64, 64)), (t, (16, 64, 64))), ((t, (32, 64, 64)), (t, (40, 64, 64))),
                              ((t, (64, 32, 64)), (t, (64, 16, 64))), ((t, (64, 32, 64)), (t, (64, 40, 64))),
                              ((t, (64, 64, 64)), (t, (64, 64, 60))), ((t, (64, 64, 64)), (t, (64, 64, 77))),
                              ((b, (64, 512, 64)), (b, (64, 528, 64))), ((b, (64, 64, 80)), (b, (64, 64, 68))),
                              ((s, (256, 64, 64, 0)), (s, (272, 64, 64, 0))), ((s, (256, 256, 64, 1)), (s, (256, 272, 64, 1))),
                              ((s, (256, 272, 64, 0)), (s, (256, 272, 64, 1))), ((s, (64, 64, 68, 0)), (s, (64, 64, 68, 1)))]:
        assert have[accepted] == 1 and have[refused] == 0, (accepted, refused)


def test_table_reaches_every_launchable_instantiation():
    reached = set()
    for c in cases.CASES:
        reached.update(cases.instantiations(c))
    assert reached == set(cases.LAUNCHABLE), sorted(reached ^ set(cases.LAUNCHABLE))
    assert len(cases.LAUNCHABLE) == 5 + 6 + 16 + 8 + 8
    # the persistent runs go through all five stream instantiations at 2, 3 (== stages) and 4 k-tiles
    stream = {"tgemm_stream_kernel<%s, %s, %s>" % (("true" if op == "dgrad" else "false"), ("true" if a else "false"),
                                                     ("true" if s else "false")) for op, a, _, s in cases.STREAM_INSTANTIATIONS}
    assert stream == {n for n in cases.LAUNCHABLE if n.startswith("tgemm_stream_kernel")}
    assert [k // 16 for k in cases.PERSISTENT_K] == [2, 3, 4] and cases.PERSISTENT_M % 128 not in (0, cases.PERSISTENT_M)


def test_launched_rows_stand_on_the_accepted_side_of_every_limit_and_refusals_on_the_other():
    g = cases.GEMM_CASES
    assert any(c.Co == 32 for c in g) and any(c.Ci == 32 for c in g) and any(c.L == 64 for c in g)
    assert any(c.affine and c.op == "fwd" and not c.stats and c.Ci == 512 for c in g)
    assert any(c.stats and c.Co == 256 for c in g) and any(c.stats and c.affine and c.Ci == 256 for c in g)
    refused = {}
    for r in cases.REJECTS:
        base = cases.BY_ID[r.base]
        refused.setdefault((base.op, base.affine, base.stats), []).append(r)

    def has(key, **override):
        return any(r.override == override for r in refused.get(key, []))
    assert has(("fwd", 0, 0), Co=16) and has(("fwd", 0, 0), Co=40) and has(("fwd", 0, 0), Ci=16) and has(("fwd", 0, 0), Ci=40)
    assert has(("fwd", 0, 0), L=60) and has(("fwd", 0, 0), L=77)
    assert has(("wgrad", 0, 0), L=68) and has(("wgrad", 1, 0), L=68)
    assert has(("fwd", 1, 0), Ci=528) and has(("fwd", 0, 1), Co=272) and has(("fwd", 1, 1), Ci=272)
    faults = {(cases.BY_ID[r.base].op, r.fault) for r in cases.REJECTS if r.fault}
    assert {("fwd", "misaligned"), ("dgrad", "misaligned"), ("wgrad", "misaligned"), ("fwd", "null_ticket"),
            ("dgrad", "null_ticket"), ("wgrad", "null_workspace")} <= faults
    # a refused shape really is one: the predicates say so (the entry points consult exactly these)
    for r in cases.REJECTS:
        base = cases.BY_ID[r.base]
        if not r.override or base.op not in ("fwd", "dgrad", "wgrad"):
            continue
        d = dict(Co=base.Co, Ci=base.Ci, L=base.L)
        d.update(r.override)
        ok = q("regnet_conv1x1_train_supported", d["Co"], d["Ci"], d["L"])
        if base.op == "wgrad":
            ok = ok and d["L"] % 16 == 0
        if base.stats:
            ok = ok and q("regnet_conv1x1_fwd_stats_supported", d["Co"], d["Ci"], d["L"], base.affine)
        elif base.affine:
            ok = ok and q("regnet_conv1x1_bnrelu_supported", d["Co"], d["Ci"], d["L"])
        assert not ok, r.id


def test_table_covers_the_tile_edges():
    fwd = [c for c in cases.GEMM_CASES if c.op == "fwd"]
    assert {c.Co for c in fwd} >= {32, 48, 128, 144, 160, 256, 272, 1024}
    assert {c.Ci for c in cases.GEMM_CASES if c.op == "dgrad"} >= {32, 48, 128, 144, 160, 256}
    for rows in (fwd, [c for c in cases.GEMM_CASES if c.op == "dgrad"]):
        assert {c.L for c in rows} >= {64, 256, 260, 508, 4112}
        assert {(c.Ci if c.op == "fwd" else c.Co) for c in rows} >= {32, 48, 64, 512}
    assert all(c.Co != 272 or not c.stats for c in fwd)
    for affine, stats in ((1, 0), (0, 1), (1, 1)):
        rows = [c for c in fwd if (c.affine, c.stats) == (affine, stats)]
        assert {c.Ci // 16 for c in rows} >= {2, 3, 4}, (affine, stats)
        assert any(c.Co % 128 and c.Co > 128 for c in rows) and any(c.L % 256 for c in rows)
        assert not affine or {c.relu for c in rows} == {0, 1}
    w = [c for c in cases.GEMM_CASES if c.op == "wgrad"]
    assert {c.Ci for c in w} >= {48, 128, 144, 256, 272} and {c.Co for c in w} >= {48, 160}
    assert any(c.B == 1 and c.L == 64 and c.slices == 1 and not c.workspace for c in w)
    assert any(c.B == 2 and c.L == 64 and c.slices == 1 and c.workspace for c in w)
    assert any(c.L == 4112 and c.slices == 1 for c in w) and any(c.L == 8192 and c.B == 1 and c.slices == 32 for c in w)
    for tile_n in (128, 256):
        assert {(c.affine, c.relu) for c in w if c.tile_n == tile_n} >= {(0, 0), (1, 0), (1, 1)}, tile_n
        assert any(c.slices > 1 for c in w if c.tile_n == tile_n and c.affine)
        assert any(c.slices > 1 for c in w if c.tile_n == tile_n and not c.affine)


def test_table_covers_the_small_channel_kernels():
    s = [c for c in cases.SMALL_CASES if c.op == "smallci"]
    assert {(c.Ci, c.Co, c.stats) for c in s} == {(ci, co, st) for ci in range(1, 9) for co in (1, 20, 128) for st in (0, 1)}
    o = [c for c in cases.SMALL_CASES if c.op == "smallco"]
    assert {(c.Co, c.direction, c.bias) for c in o} == {(co, d, b) for co in range(1, 5) for d in (0, 1) for b in (0, 1)}
    w = [c for c in cases.SMALL_CASES if c.op == "wgrad_smallci"]
    assert {(c.Ci, c.Co) for c in w} == {(ci, co) for ci in range(1, 9) for co in (1, 4, 5, 18)}
    for rows in (s, o, w):
        assert {c.L for c in rows} >= set(cases.SMALL_L) and all(c.L % 4 == 0 for c in rows)
    assert {c.L for c in s if c.stats} == set(cases.SMALL_L)      # the partly live blocks with statistics on
    # the slice rule by hand against the library's count of partial matrices, and the slices the rows are there for
    for c in w:
        S = cases.smallci_wgrad_slices(c.B, c.Co, c.L)
        assert q("regnet_conv1x1_wgrad_smallci_partials", c.B, c.Co, c.L) == c.B * S, c.id
        assert S == {4: 1, 1020: 1, 1028: 1, 4100: 2, 8196: 3, 4096 * 1024 + 4: 1024}[c.L], c.id
        if S > 1:
            assert S * cases.smallci_wgrad_slice_len(c.B, c.Co, c.L) > c.L      # the rounded length passes L


def test_trailing_empty_slices_of_the_small_weight_gradient():
    """While the slice count is ceil(L / 4096) every slice starts below L, whatever the rounding to whole wave steps; held by the
    1024-workgroup aim instead it leaves trailing slices empty: the table has one such row."""
    for B, Co in ((1, 1), (2, 18), (8, 128), (64, 64), (1, 2048)):
        for L in list(range(4, 20000, 4)) + [61444, 65540, 69636, 4096 * 40 + 4]:
            S = cases.smallci_wgrad_slices(B, Co, L)
            if S == (L + 4095) // 4096:
                assert (S - 1) * cases.smallci_wgrad_slice_len(B, Co, L) < L, (B, Co, L)
    c = cases.BY_ID["wgrad-smallci-empty-slices"]
    S, n = cases.smallci_wgrad_slices(c.B, c.Co, c.L), cases.smallci_wgrad_slice_len(c.B, c.Co, c.L)
    assert (S, n) == (1024, 4352) and S - (c.L + n - 1) // n == 60
    assert q("regnet_conv1x1_wgrad_smallci_partials", c.B, c.Co, c.L) == 1024
