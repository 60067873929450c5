"""The case table of the plain-layer GEMM tests (tests/gemm2_cases.py) against ``regnet_mlp_layer_plan``, the host function the
launcher of regnet_mlp_layer_f32 takes its tile and grid from: every row is dispatched to the configuration it is there for
and has the tail / slab / padding properties it names, and the table as a whole covers what tests/test_gpu_gemm2_tiles.py is
meant to exercise.  No GPU."""
import ctypes

import pytest

from . import gemm2_cases as cases

OK, ERR_SHAPE, ERR_NULL, ERR_UNSUPPORTED = 0, -1, -2, -3


@pytest.mark.parametrize("case", cases.CASES, ids=[c.id for c in cases.CASES])
def test_row_takes_its_configuration_with_its_features(case):
    assert case.K % 4 == 0 and case.pool in (0, 64) and case.ldc_pad in (1, 4)
    plan = cases.plan_of(case)
    assert plan["config"] == case.config, plan
    have = cases.features_of(case, plan)
    assert case.features <= have, "%s: the plan does not give %s (%s)" % (case.id, sorted(case.features - have), plan)
    # every property is named in the row (nothing is covered by accident)
    assert have == case.features, "%s: unnamed %s" % (case.id, sorted(have - case.features))
    # slab sums exactly where the dispatch comment says: the 64 x 128 tile and the two-per-CU 128 x 128 tile
    assert plan["slab_kt"] == (8 if case.config in "AC" else 0)
    # outputs stay small enough for a case to take seconds
    assert (case.P // 64 if case.pool else case.P) * (case.N + case.ldc_pad) * 4 <= 150e6


def _covered(config):
    return [(c, c.features) for c in cases.CASES if c.config == config]


def test_table_covers_the_tail_and_column_edges_of_the_large_tiles():
    for config in "CDE":
        feats = [f for _, f in _covered(config)]
        # (one round -- tiles <= slots -- is reachable for C only: D and E are taken from four rounds of the CUs up)
        assert any(f & ({"fits_slots"} if config == "C" else {"fits_slots", "rem_zero", "rem_above_half"}) for f in feats), config
        assert any("rem_above_half" in f for f in feats), config
        assert any({"tail", "slice_beyond_P"} <= f for f in feats), config
        assert any({"tail", "ragged_N"} <= f for f in feats), config
    assert any("rem_zero" in f for _, f in _covered("D"))
    for config in "DE":
        pooled = [c for c, f in _covered(config) if "pool_single" in f]
        assert pooled and all(c.pool == 64 and (c.P // 64) % 2 == 1 for c in pooled), config
        assert all(cases.plan_of(c)["tail_tiles"] == 0 for c in pooled)   # pooling never splits
    assert any(c.pool and cases.kpad(c) >= 256 for c, _ in _covered("E"))   # pooled keeps E where plain rows take C


def test_table_covers_the_small_kernels():
    a = [c for c, _ in _covered("A")]
    assert any(c.P == 1 for c in a) and any(c.N == 1 for c in a) and any(c.N == 129 for c in a)
    assert any(c.pool for c in a) and any(cases.kpad(c) == 32 for c in a)
    assert any(cases.kpad(c) == 272 and "open_slab" in c.features for c in a)   # two full slabs and an open one
    m = [c for c, _ in _covered("M")]
    assert {c.K for c in m} >= {4, 12, 16} and all(cases.kpad(c) == 16 for c in m)
    assert any(c.P % 128 and c.N % 128 for c in m) and any(c.pool for c in m)
    c_ = [c for c, _ in _covered("C")]
    assert any(cases.kpad(c) == 256 and "two_full_slabs" in c.features for c in c_)
    assert any(cases.kpad(c) == 272 and "open_slab" in c.features for c in c_)


def test_every_configuration_has_ragged_k_both_relu_values_and_both_row_alignments():
    for config in "ACDEM":
        rows = [c for c, _ in _covered(config)]
        assert any("Ka_ragged" in c.features for c in rows), config
        assert {c.relu for c in rows} == {0, 1}, config
        assert {c.ldc_pad for c in rows} == {1, 4}, config
    assert abs(sum(c.ldc_pad == 4 for c in cases.CASES) * 2 - len(cases.CASES)) <= 2   # half and half
    assert len({c.id for c in cases.CASES}) == len(cases.CASES)


def test_bit_identity_pair_is_a_c_case_and_an_a_call():
    """test_gpu_gemm2_tiles compares the first 1000 rows of every C case with a P = 1000 call of the same layer: that call has
    to be configuration A for the comparison to be between two kernels."""
    for c, _ in _covered("C"):
        rc, plan = cases.query_plan(1000, c.N, cases.kpad(c), 0)
        assert rc == OK and plan["config"] == "A" and plan["slab_kt"] == 8, (c.id, plan)


def test_plan_returns_the_layers_own_error_codes():
    q = cases.query_plan
    zero = dict.fromkeys(("tile_rows", "tile_cols", "waves", "wg_per_cu", "slab_kt", "main_blocks", "tail_tiles", "tail_split"), 0)
    for args, want in [((-1, 128, 32, 0), ERR_SHAPE), ((64, 0, 32, 0), ERR_SHAPE), ((64, 128, 0, 0), ERR_SHAPE),
                       ((64, 128, 40, 0), ERR_SHAPE), ((64, 128, 32, 32), ERR_UNSUPPORTED), ((65, 128, 32, 64), ERR_UNSUPPORTED),
                       ((0, 128, 32, 0), OK), ((0, 128, 32, 64), OK)]:
        rc, plan = q(*args)
        assert rc == want, args
        assert {k: plan[k] for k in zero} == zero and plan["config"] == "M", args   # nothing reported
    # a shape error wins over an unsupported pooling, as in regnet_mlp_layer_f32
    assert q(65, 128, 40, 64)[0] == ERR_SHAPE
    from regnet_for_3d_grasping_amd import _lib
    assert _lib.call("regnet_mlp_layer_plan", None, 64, 128, 32, 0, None) == ERR_NULL
    # Kpad == 16: one block per 128 x 128 tile, nothing else set
    rc, plan = q(300, 130, 16, 0)
    assert rc == OK and plan["config"] == "M" and plan["main_blocks"] == 3 * 2 and plan["tail_tiles"] == 0
    # the grid of the tile kernels is main_blocks + tail_tiles * tail_split
    rc, plan = q(131000, 128, 64, 0)
    assert rc == OK and (plan["main_blocks"], plan["tail_tiles"], plan["tail_split"]) == (768, 256, 2)


def test_plan_needs_no_device_pointer():
    """Host memory in, host memory out: the eight words are all the function touches."""
    buf = (ctypes.c_int64 * 10)(*([-5] * 10))
    from regnet_for_3d_grasping_amd import _lib
    assert _lib.call("regnet_mlp_layer_plan", None, 4096, 256, 128, 0, ctypes.addressof(buf) + 8) == OK
    assert buf[0] == -5 and buf[9] == -5 and list(buf[1:5]) == [64, 128, 4, 4]
