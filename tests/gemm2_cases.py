"""The shapes at which the plain-layer GEMM (csrc/gemm2.h, dispatched by csrc/mlp.hip: plan_gemm2) is tested, one table for
tests/test_gemm2_plan_cpu.py (does the library take the configuration each row is there for, and does the table cover what it
has to) and tests/test_gpu_gemm2_tiles.py (the kernels at these shapes).

Configurations, as ``regnet_mlp_layer_plan`` reports them (tile rows, tile columns, waves, workgroups per CU):
    D (256, 128, 8, 2)   C (128, 128, 4, 2)   E (128, 128, 4, 3)   A (64, 128, 4, 4)   M (0, 0, 0, 0) = mlp_gemm_kernel<0>
``features`` of a row are properties ``features_of`` derives from the library's plan of that row -- never from a copy of the
thresholds -- so a retuned dispatch fails the CPU test instead of silently moving a row to another kernel:
    fits_slots        one round: tiles <= workgroup slots (256 CUs x workgroups per CU), nothing split
    rem_zero          several rounds, the last one full, nothing split
    rem_above_half    several rounds, the last partial one fills more than half the slots, nothing split
    tail              the last partial round is cut into half-height slices
    slice_beyond_P    tail, and the last row tile holds fewer valid rows than half a tile: its slice 1 starts beyond P
    ragged_N          N % 128 != 0
    pool_single       pooled, P % tile rows == 64: the last tile holds a single neighbourhood
    open_slab         slab sums, Kpad > 128 and not a multiple of 128: full slabs plus an open one
    two_full_slabs    slab sums, Kpad == 256: two slabs, nothing open
    Ka_ragged         Ka < Kpad and Ka % 16 != 0: the last k-tile is partly zero columns
"""
import collections
import os

_SWITCHES = [v for v in ("REGNET_G2_TILE", "REGNET_G2_T8", "REGNET_GEMM2") if v in os.environ]
if _SWITCHES:
    raise RuntimeError("%s set in the environment: the launcher reads these A/B switches once per process and the case table "
                       "of tests/gemm2_cases.py describes the default dispatch -- unset them to run the gemm2 tile tests"
                       % ", ".join(_SWITCHES))

CONFIGS = {(256, 128, 8, 2): "D", (128, 128, 4, 2): "C", (128, 128, 4, 3): "E", (64, 128, 4, 4): "A", (0, 0, 0, 0): "M"}
CUS = 256

# K is Ka (a multiple of 4); Kpad = ceil16(K).  relu is the float test's setting (the exact test runs the other one);
# ldc = N + ldc_pad (4: rows stay 16-byte aligned, 1: they do not).
Case = collections.namedtuple("Case", "id config P N K pool relu ldc_pad features")
CASES = [
    # 1024 tiles = two full rounds
    Case("D-rem0", "D", 32768, 1024, 32, 0, 1, 4, {"rem_zero"}),
    # 130 x 8 = 1040 tiles, the last 16 split; the last row tile holds 100 of 256 rows
    Case("D-tail-beyondP-raggedN", "D", 33124, 1000, 260, 0, 0, 1, {"tail", "slice_beyond_P", "ragged_N", "Ka_ragged"}),
    Case("D-pool", "D", 64 * 2049, 256, 32, 64, 1, 1, {"pool_single"}),
    # 427 x 3 = 1281 tiles, remainder 257 of 512 slots; the last column tile holds one column
    Case("D-rem-above-half", "D", 109200, 257, 32, 0, 0, 4, {"rem_above_half", "ragged_N"}),
    # 129 x 2 = 258 tiles
    Case("C-fits", "C", 16400, 256, 256, 0, 1, 4, {"fits_slots", "two_full_slabs"}),
    # 172 x 3 = 516 tiles, the last 4 split; the last row tile holds 40 of 128 rows
    Case("C-tail-beyondP-raggedN", "C", 21928, 380, 260, 0, 0, 1,
         {"tail", "slice_beyond_P", "ragged_N", "Ka_ragged", "open_slab"}),
    # 260 x 3 = 780 tiles, remainder 268
    Case("C-rem-above-half", "C", 33200, 384, 272, 0, 1, 1, {"rem_above_half", "open_slab"}),
    # 1024 tiles, remainder 256 of 768 slots split; the last row tile holds 56 rows
    Case("E-tail-beyondP", "E", 131000, 128, 64, 0, 1, 4, {"tail", "slice_beyond_P"}),
    # 1500 tiles, remainder 732
    Case("E-rem-above-half", "E", 192000, 128, 48, 0, 0, 1, {"rem_above_half"}),
    Case("E-pool-K256", "E", 64 * 2047, 128, 256, 64, 0, 4, {"pool_single"}),
    # N > 128 below four rounds of the 256-row tile: 512 x 2 = 1024 tiles, remainder 256 split
    Case("E-tail-raggedN", "E", 65500, 200, 36, 0, 1, 1, {"tail", "ragged_N", "Ka_ragged"}),
    Case("A-P1-N1-K32", "A", 1, 1, 32, 0, 1, 1, {"fits_slots", "ragged_N"}),
    Case("A-N129-open-slab", "A", 200, 129, 260, 0, 0, 4, {"fits_slots", "ragged_N", "open_slab", "Ka_ragged"}),
    Case("A-pool", "A", 64 * 5, 129, 36, 64, 1, 4, {"ragged_N", "Ka_ragged"}),
    Case("A-blocks", "A", 777, 384, 516, 0, 1, 1, {"fits_slots", "open_slab", "Ka_ragged"}),
    Case("M-K4-ragged", "M", 130, 130, 4, 0, 1, 1, {"ragged_N", "Ka_ragged"}),
    Case("M-K12-N1", "M", 257, 1, 12, 0, 0, 4, {"ragged_N", "Ka_ragged"}),
    Case("M-K16-interior", "M", 128, 128, 16, 0, 0, 4, set()),
    Case("M-pool", "M", 64 * 3, 130, 12, 64, 1, 1, {"ragged_N", "Ka_ragged"}),
]
BY_ID = {c.id: c for c in CASES}


def kpad(case):
    return (case.K + 15) // 16 * 16


def query_plan(P, N, Kpad, pool):
    """``regnet_mlp_layer_plan`` -> (status, dict of its eight outputs + the configuration's letter, None if unknown)."""
    import ctypes
    from regnet_for_3d_grasping_amd import _lib
    out = (ctypes.c_int64 * 8)()
    rc = _lib.call("regnet_mlp_layer_plan", None, P, N, Kpad, pool, ctypes.addressof(out))
    names = ("tile_rows", "tile_cols", "waves", "wg_per_cu", "slab_kt", "main_blocks", "tail_tiles", "tail_split")
    plan = dict(zip(names, [int(v) for v in out]))
    plan["config"] = CONFIGS.get(tuple(plan[n] for n in names[:4]))
    return rc, plan


def plan_of(case):
    rc, plan = query_plan(case.P, case.N, kpad(case), case.pool)
    assert rc == 0, (case.id, rc)
    return plan


def features_of(case, plan):
    """The properties of the module docstring that hold for ``case`` under the library's ``plan`` of it."""
    out = set()
    Kp = kpad(case)
    if case.N % 128:
        out.add("ragged_N")
    if case.K < Kp and case.K % 16:
        out.add("Ka_ragged")
    if plan["config"] == "M":
        return out
    rows = plan["tile_rows"]
    tiles = ((case.P + rows - 1) // rows) * ((case.N + plan["tile_cols"] - 1) // plan["tile_cols"])
    slots = CUS * plan["wg_per_cu"]
    assert plan["main_blocks"] + plan["tail_tiles"] == tiles, (case.id, plan)
    assert plan["tail_split"] == (2 if plan["tail_tiles"] else 0), (case.id, plan)
    if plan["tail_tiles"]:
        assert 0 < plan["tail_tiles"] == tiles % slots <= slots // 2 and not case.pool, (case.id, plan)
        out.add("tail")
        if case.P % rows and case.P % rows < rows // 2:
            out.add("slice_beyond_P")
    elif not case.pool:
        if tiles <= slots:
            out.add("fits_slots")
        elif tiles % slots == 0:
            out.add("rem_zero")
        elif tiles % slots > slots // 2:
            out.add("rem_above_half")
    if case.pool and case.P % rows == 64:
        out.add("pool_single")
    if plan["slab_kt"]:
        assert plan["slab_kt"] == 8, (case.id, plan)
        if Kp > 128 and Kp % 128:
            out.add("open_slab")
        if Kp == 256:
            out.add("two_full_slabs")
    return out
