"""The shapes at which the training GEMM (csrc/tgemm.hip: the forward, input gradient and weight gradient of every 1x1 convolution
of a training step) is tested, one table for tests/test_tgemm_plan_cpu.py (does the library's host side agree with what each row
expects, and does the table cover what it has to) and tests/test_gpu_tgemm_tiles.py (the kernels at these shapes).

Everything here is written by hand from the rules in csrc/tgemm.hip and include/regnet_hip.h; nothing is computed by calling the
library, so a retuned rule fails the CPU test instead of silently moving a row to another kernel.

    op             entry points                                                  kernel
    fwd            regnet_conv1x1_fwd_stream_f32 and regnet_conv1x1_fwd_f32      stream<row> and tile<row, kmaj, 256>
    fwd, affine    regnet_conv1x1_fwd_bnrelu_stream_f32                          stream<row, affine>
    fwd, stats     regnet_conv1x1_fwd_stats_stream_f32 (scale NULL or not)       stream<row, [affine,] stats>
    dgrad          regnet_conv1x1_dgrad_stream_f32 and regnet_conv1x1_dgrad_f32  stream<kmaj> and tile<kmaj, kmaj, 256>
    wgrad          regnet_conv1x1_wgrad_f32 / regnet_conv1x1_wgrad_bnrelu_f32    tile<row, row, 128 | 256, plain | affine> + reduce
    smallci        regnet_conv1x1_fwd_smallci_f32 / ..._stats_f32                conv_smallci_kernel<Ci, stats>
    smallco        regnet_conv1x1_smallco_f32, dir 0 (forward) / 1 (input grad)  conv_smallco_fwd / dgrad_kernel<Co>
    wgrad_smallci  regnet_conv1x1_wgrad_smallci_f32                              wgrad_smallci_kernel<Ci>

Limits (both sides of each are in LIMITS and, as launches and refusals, in CASES and REJECTS):
    Co, Ci   multiples of 16 from 32 up             16 | 32, and 40
    L        a multiple of 4 from 64 up             60 | 64, and 77;   the weight gradient and an affine operand: L % 16 == 0
    affine   Ci <= 512 (TG_AFF_MAXK)                512 | 528
    stats    Co <= 256 (TG_STAT_MAXM)               256 | 272;         with an affine operand Ci <= 256 (TG_STAT_AFF_MAXK): 256 | 272

The output tile is 128 channels x 256 points (weight gradient: 128 x 128 when Ci <= 128, else 128 x 256), a k-tile is 16 deep and
the ring has three stages: M = 32 / 48 (one partial tile), 128 (exact), 144 / 160 (a second, partial tile), 256, 272, 1024;
L = 64 (one partial tile), 256 (exact), 260 (a tail of one 16-byte chunk), 508 (a tail of 252), 4112 / 272 (L % 256 == 16),
496 (a tail of 240 with L % 16 == 0); K = 32 (two k-tiles: the next tile is drawn in the prologue), 48 (as many as stages), 64, 512.

Weight gradient slices (regnet_conv1x1_wgrad_slices): tiles = ceil(Co / 128) * ceil(Ci / 256); S doubles from 1 while the halved
slice L / (2 S) is whole, a multiple of 16 and >= 256 points, and S * tiles * B < 256.  n = B * S partial matrices; n == 1 stores
straight to dW and needs no workspace.
"""
import collections

# slices / tile_n / workspace: weight gradient rows only (None elsewhere).  direction / bias: smallco rows only.
Case = collections.namedtuple("Case", "id op affine relu stats B Co Ci L why slices tile_n workspace direction bias")


def _c(id, op, B, Co, Ci, L, why, affine=0, relu=0, stats=0, slices=None, tile_n=None, workspace=None, direction=None, bias=None):
    return Case(id, op, affine, relu, stats, B, Co, Ci, L, why, slices, tile_n, workspace, direction, bias)


GEMM_CASES = [
    # ---- forward, plain: the stream kernel and the one-workgroup-per-tile kernel (bit-identical)
    _c("fwd-Co32-K32-L64", "fwd", 2, 32, 32, 64, "every lower limit at once: one partial tile, two k-tiles"),
    _c("fwd-Co48-K48-L256", "fwd", 2, 48, 48, 256, "an exact point tile, as many k-tiles as stages"),
    _c("fwd-Co128-K64-L260", "fwd", 3, 128, 64, 260, "an exact channel tile, a point tail of one 16-byte chunk"),
    _c("fwd-Co144-K512-L508", "fwd", 2, 144, 512, 508, "a second channel tile of 16 rows, a tail of 252, 32 k-tiles"),
    _c("fwd-Co160-K32-L4112", "fwd", 2, 160, 32, 4112, "17 point tiles, L % 256 == 16"),
    _c("fwd-Co256-K48-L64", "fwd", 3, 256, 48, 64, "two exact channel tiles"),
    _c("fwd-Co1024-K64-L260", "fwd", 1, 1024, 64, 260, "eight channel tiles"),
    _c("fwd-Co272-K32-L508", "fwd", 2, 272, 32, 508, "a third channel tile of 16 rows (no statistics at this width)"),
    # ---- forward with the operand's BatchNorm (+ ReLU) on the fragment
    _c("aff-Co32-K32-L64-relu", "fwd", 2, 32, 32, 64, "the lower limits", affine=1, relu=1),
    _c("aff-Co48-K48-L256", "fwd", 2, 48, 48, 256, "no ReLU: the lower clamp is -inf", affine=1, relu=0),
    _c("aff-Co144-K512-L496-relu", "fwd", 2, 144, 512, 496, "the largest affine table (Ci == 512), a tail of 240", affine=1, relu=1),
    _c("aff-Co160-K64-L4112", "fwd", 2, 160, 64, 4112, "17 point tiles, L % 256 == 16, no ReLU", affine=1, relu=0),
    _c("aff-Co1024-K32-L272-relu", "fwd", 1, 1024, 32, 272, "eight channel tiles", affine=1, relu=1),
    _c("aff-Co256-K48-L64", "fwd", 3, 256, 48, 64, "two exact channel tiles, no ReLU", affine=1, relu=0),
    # ---- forward leaving the statistics of the BatchNorm that follows
    _c("stat-Co32-K32-L64", "fwd", 2, 32, 32, 64, "the lower limits: 96 of 128 table rows unused", stats=1),
    _c("stat-Co48-K48-L260", "fwd", 3, 48, 48, 260, "a point tail of 4: the column masks of the sums", stats=1),
    _c("stat-Co128-K64-L508", "fwd", 2, 128, 64, 508, "an exact channel tile, the last 4 columns masked", stats=1),
    _c("stat-Co144-K512-L256", "fwd", 2, 144, 512, 256, "the row mask of the sums (16 of 128 rows), 32 k-tiles", stats=1),
    _c("stat-Co160-K32-L4112", "fwd", 2, 160, 32, 4112, "34 tiles per scene", stats=1),
    _c("stat-Co256-K48-L64", "fwd", 3, 256, 48, 64, "the whole table (Co == 256)", stats=1),
    _c("affstat-Co32-K32-L64-relu", "fwd", 2, 32, 32, 64, "the lower limits", affine=1, relu=1, stats=1),
    _c("affstat-Co160-K48-L272", "fwd", 3, 160, 48, 272, "a second point tile of 16 columns, no ReLU", affine=1, relu=0, stats=1),
    _c("affstat-Co256-K256-L4112-relu", "fwd", 2, 256, 256, 4112, "both tables full (Co == 256, Ci == 256)", affine=1, relu=1, stats=1),
    _c("affstat-Co48-K64-L496", "fwd", 2, 48, 64, 496, "a tail of 240, no ReLU", affine=1, relu=0, stats=1),
    # ---- input gradient: M = Ci (the clamped m chunk of the k-major A operand), K = Co
    _c("dgrad-Ci32-K32-L64", "dgrad", 2, 32, 32, 64, "the lower limits"),
    _c("dgrad-Ci48-K48-L260", "dgrad", 3, 48, 48, 260, "a partial m chunk row, a tail of one chunk"),
    _c("dgrad-Ci128-K64-L256", "dgrad", 2, 64, 128, 256, "exact tiles"),
    _c("dgrad-Ci144-K512-L508", "dgrad", 2, 512, 144, 508, "a second channel tile of 16 rows, 32 k-tiles"),
    _c("dgrad-Ci160-K32-L4112", "dgrad", 2, 32, 160, 4112, "34 tiles per scene"),
    _c("dgrad-Ci256-K48-L64", "dgrad", 3, 48, 256, 64, "two exact channel tiles"),
    # ---- weight gradient (slices, tile width and workspace by hand from the rule in the module docstring)
    _c("wgrad-n1", "wgrad", 1, 48, 48, 64, "n == 1: straight to dW, NULL workspace", slices=1, tile_n=128, workspace=False),
    _c("wgrad-scenes-only", "wgrad", 2, 160, 128, 64, "the reduction goes over scenes only; an exact 128-wide tile",
       slices=1, tile_n=128, workspace=True),
    _c("wgrad-odd-L", "wgrad", 2, 48, 144, 4112, "L / 2 is no multiple of 16: one slice; 144 of 256 columns",
       slices=1, tile_n=256, workspace=True),
    _c("wgrad-many-slices", "wgrad", 1, 160, 272, 8192, "32 slices of 256 points; second row and column tiles of 32 and 16",
       slices=32, tile_n=256, workspace=True),
    _c("wgrad-many-slices-narrow", "wgrad", 1, 48, 48, 8192, "32 slices on the 128-wide tile", slices=32, tile_n=128, workspace=True),
    _c("wgrad-blocks-stop", "wgrad", 32, 256, 272, 1024, "halving stops at 256 workgroups (2 x 4 x 32), not at the slice length",
       slices=2, tile_n=256, workspace=True),
    _c("wgrad-length-stop", "wgrad", 3, 160, 256, 1024, "halving stops at slices of 256 points; an exact 256-wide tile",
       slices=4, tile_n=256, workspace=True),
    _c("wgrad-aff-n1-relu", "wgrad", 1, 48, 128, 64, "affine, n == 1", affine=1, relu=1, slices=1, tile_n=128, workspace=False),
    _c("wgrad-aff-narrow", "wgrad", 2, 160, 48, 1024, "affine without ReLU (lower clamp -inf) on the 128-wide tile",
       affine=1, relu=0, slices=4, tile_n=128, workspace=True),
    _c("wgrad-aff-wide-relu", "wgrad", 2, 48, 272, 4112, "affine + ReLU, a second column tile of 16 (scale rows clamped)",
       affine=1, relu=1, slices=1, tile_n=256, workspace=True),
    _c("wgrad-aff-wide", "wgrad", 3, 160, 144, 512, "affine without ReLU on the 256-wide tile", affine=1, relu=0,
       slices=2, tile_n=256, workspace=True),
    _c("wgrad-aff-256-relu", "wgrad", 1, 48, 256, 8192, "affine + ReLU, 32 slices", affine=1, relu=1, slices=32, tile_n=256,
       workspace=True),
]

# ---- the small-channel kernels.  L: 4 = a one-thread block; 1020 = a block that is partly live (255 threads); 1028 = a second block
# with one live thread (with statistics on it still takes part in the block's sums); 4100 / 8196 = five / nine blocks, and in the
# weight gradient two / three slices whose length, rounded up to whole wave steps, passes L.  Trailing EMPTY slices need the slice
# count to be held by the 1024-workgroup aim instead of by L / 4096 (while slices == ceil(L / 4096) every slice starts below L):
# B = 1, Co <= 16 and L = 4096 * 1024 + 4 give 1024 slices of 4352 points, of which the last 60 start beyond L.
SMALL_L = [4, 1020, 1028, 4100, 8196]
SMALL_CASES = []
for _ci in range(1, 9):
    for _k, _co in enumerate((1, 20, 128)):
        for _stats in (0, 1):
            _L = SMALL_L[(_ci + _k + 2 * _stats) % 5]
            SMALL_CASES.append(_c("smallci-Ci%d-Co%d-L%d%s" % (_ci, _co, _L, "-stats" if _stats else ""), "smallci", 2, _co, _ci, _L,
                                  "conv_smallci_kernel<%d, %s>" % (_ci, "true" if _stats else "false"), stats=_stats))
for _co in range(1, 5):
    for _dir in (0, 1):
        for _bias in (0, 1):
            _L = SMALL_L[(_co + 2 * _dir + _bias) % 5]
            _ci = (20, 128, 7, 33)[(_co + _dir + _bias) % 4]
            SMALL_CASES.append(_c("smallco-Co%d-Ci%d-L%d-%s%s" % (_co, _ci, _L, "dgrad" if _dir else "fwd", "-bias" if _bias else ""),
                                  "smallco", 2, _co, _ci, _L, "conv_smallco_%s_kernel<%d>" % ("dgrad" if _dir else "fwd", _co),
                                  direction=_dir, bias=_bias))
for _ci in range(1, 9):
    for _k, _co in enumerate((1, 4, 5, 18)):
        _L = SMALL_L[(_ci + _k) % 5]
        SMALL_CASES.append(_c("wgrad-smallci-Ci%d-Co%d-L%d" % (_ci, _co, _L), "wgrad_smallci", 2, _co, _ci, _L,
                              "wgrad_smallci_kernel<%d>; the last wave owns %d of four rows" % (_ci, (_co - 1) % 4 + 1)))
SMALL_CASES.append(_c("wgrad-smallci-empty-slices", "wgrad_smallci", 1, 5, 3, 4096 * 1024 + 4,
                      "1024 slices of 4352 points: the last 60 are empty and write zeros"))

CASES = GEMM_CASES + SMALL_CASES
BY_ID = {c.id: c for c in CASES}

# ---- the persistent path of the stream kernel: (op, affine, relu, stats) x K.  The test reserves as many workgroup slots as the
# chip has CUs, so the grid is min(total, CUs), and chooses B and L at run time: total = grid, grid + 1 and about 2.5 grid.
STREAM_INSTANTIATIONS = [("fwd", 0, 0, 0), ("fwd", 1, 1, 0), ("fwd", 0, 0, 1), ("fwd", 1, 0, 1), ("dgrad", 0, 0, 0)]
PERSISTENT_K = [32, 48, 64]          # 2, 3 (== stages) and 4 k-tiles
PERSISTENT_M = 160                   # a second channel tile of 32 rows

# ---- both sides of every limit of the host-side predicates: (function, arguments, expected value)
LIMITS = [
    ("regnet_conv1x1_train_supported", (16, 64, 64), 0), ("regnet_conv1x1_train_supported", (32, 64, 64), 1),
    ("regnet_conv1x1_train_supported", (40, 64, 64), 0),
    ("regnet_conv1x1_train_supported", (64, 16, 64), 0), ("regnet_conv1x1_train_supported", (64, 32, 64), 1),
    ("regnet_conv1x1_train_supported", (64, 40, 64), 0),
    ("regnet_conv1x1_train_supported", (64, 64, 60), 0), ("regnet_conv1x1_train_supported", (64, 64, 64), 1),
    ("regnet_conv1x1_train_supported", (64, 64, 77), 0), ("regnet_conv1x1_train_supported", (64, 64, 68), 1),
    ("regnet_conv1x1_bnrelu_supported", (64, 512, 64), 1), ("regnet_conv1x1_bnrelu_supported", (64, 528, 64), 0),
    ("regnet_conv1x1_bnrelu_supported", (64, 64, 68), 0), ("regnet_conv1x1_bnrelu_supported", (64, 64, 80), 1),
    ("regnet_conv1x1_bnrelu_supported", (16, 64, 64), 0), ("regnet_conv1x1_bnrelu_supported", (64, 64, 60), 0),
    ("regnet_conv1x1_fwd_stats_supported", (256, 64, 64, 0), 1), ("regnet_conv1x1_fwd_stats_supported", (272, 64, 64, 0), 0),
    ("regnet_conv1x1_fwd_stats_supported", (256, 256, 64, 1), 1), ("regnet_conv1x1_fwd_stats_supported", (256, 272, 64, 1), 0),
    ("regnet_conv1x1_fwd_stats_supported", (256, 272, 64, 0), 1), ("regnet_conv1x1_fwd_stats_supported", (64, 64, 68, 0), 1),
    ("regnet_conv1x1_fwd_stats_supported", (64, 64, 68, 1), 0), ("regnet_conv1x1_fwd_stats_supported", (64, 40, 64, 0), 0),
]

# ---- calls the entry points refuse on the host, before any launch: (id, row to take op / flags from, overrides, fault, status)
# fault: None, "misaligned" (the output pointer offset by 4 bytes), "null_ticket", "null_workspace"
ERR_SHAPE, ERR_NULL = -1, -2
Reject = collections.namedtuple("Reject", "id base override fault status")
REJECTS = [
    Reject("fwd-Co16", "fwd-Co32-K32-L64", {"Co": 16}, None, ERR_SHAPE),
    Reject("fwd-Co40", "fwd-Co32-K32-L64", {"Co": 40}, None, ERR_SHAPE),
    Reject("fwd-Ci16", "fwd-Co32-K32-L64", {"Ci": 16}, None, ERR_SHAPE),
    Reject("fwd-Ci40", "fwd-Co32-K32-L64", {"Ci": 40}, None, ERR_SHAPE),
    Reject("fwd-L60", "fwd-Co32-K32-L64", {"L": 60}, None, ERR_SHAPE),
    Reject("fwd-L77", "fwd-Co32-K32-L64", {"L": 77}, None, ERR_SHAPE),
    Reject("dgrad-Co40", "dgrad-Ci32-K32-L64", {"Co": 40}, None, ERR_SHAPE),
    Reject("dgrad-L60", "dgrad-Ci32-K32-L64", {"L": 60}, None, ERR_SHAPE),
    Reject("wgrad-L68", "wgrad-n1", {"L": 68}, None, ERR_SHAPE),
    Reject("wgrad-aff-L68", "wgrad-aff-n1-relu", {"L": 68}, None, ERR_SHAPE),
    Reject("wgrad-Ci40", "wgrad-n1", {"Ci": 40}, None, ERR_SHAPE),
    Reject("aff-Ci528", "aff-Co32-K32-L64-relu", {"Ci": 528}, None, ERR_SHAPE),
    Reject("aff-L68", "aff-Co32-K32-L64-relu", {"L": 68}, None, ERR_SHAPE),
    Reject("stat-Co272", "stat-Co32-K32-L64", {"Co": 272}, None, ERR_SHAPE),
    Reject("affstat-Ci272", "affstat-Co32-K32-L64-relu", {"Ci": 272}, None, ERR_SHAPE),
    Reject("fwd-misaligned", "fwd-Co32-K32-L64", {}, "misaligned", ERR_SHAPE),
    Reject("aff-misaligned", "aff-Co32-K32-L64-relu", {}, "misaligned", ERR_SHAPE),
    Reject("stat-misaligned", "stat-Co32-K32-L64", {}, "misaligned", ERR_SHAPE),
    Reject("dgrad-misaligned", "dgrad-Ci32-K32-L64", {}, "misaligned", ERR_SHAPE),
    Reject("wgrad-misaligned", "wgrad-n1", {}, "misaligned", ERR_SHAPE),
    Reject("fwd-null-ticket", "fwd-Co32-K32-L64", {}, "null_ticket", ERR_NULL),
    Reject("aff-null-ticket", "aff-Co32-K32-L64-relu", {}, "null_ticket", ERR_NULL),
    Reject("stat-null-ticket", "stat-Co32-K32-L64", {}, "null_ticket", ERR_NULL),
    Reject("dgrad-null-ticket", "dgrad-Ci32-K32-L64", {}, "null_ticket", ERR_NULL),
    Reject("wgrad-null-workspace", "wgrad-scenes-only", {}, "null_workspace", ERR_NULL),
    Reject("smallci-Ci9", "smallci-Ci8-Co1-L4100", {"Ci": 9}, None, ERR_SHAPE),
    Reject("smallci-L6", "smallci-Ci8-Co1-L4100", {"L": 6}, None, ERR_SHAPE),
    Reject("smallco-Co5", "smallco-Co4-Ci20-L8196-fwd", {"Co": 5}, None, ERR_SHAPE),
    Reject("wgrad-smallci-Ci9", "wgrad-smallci-Ci8-Co1-L4100", {"Ci": 9}, None, ERR_SHAPE),
]


def instantiations(case):
    """The kernel template instantiations the launchers start for ``case`` (names as in csrc/tgemm.hip)."""
    def flag(v):
        return "true" if v else "false"
    if case.op == "fwd":
        out = ["tgemm_stream_kernel<false, %s, %s>" % (flag(case.affine), flag(case.stats))]
        if not case.affine and not case.stats:
            out.append("tgemm_kernel<false, true, 256, false>")
        return out
    if case.op == "dgrad":
        return ["tgemm_stream_kernel<true, false, false>", "tgemm_kernel<true, true, 256, false>"]
    if case.op == "wgrad":
        return ["tgemm_kernel<false, false, %d, %s>" % (case.tile_n, flag(case.affine))]
    if case.op == "smallci":
        return ["conv_smallci_kernel<%d, %s>" % (case.Ci, flag(case.stats))]
    if case.op == "smallco":
        return ["conv_smallco_%s_kernel<%d>" % ("dgrad" if case.direction else "fwd", case.Co)]
    assert case.op == "wgrad_smallci", case.op
    return ["wgrad_smallci_kernel<%d>" % case.Ci]


# every instantiation the launchers of csrc/tgemm.hip can start
LAUNCHABLE = (
    ["tgemm_stream_kernel<false, false, false>", "tgemm_stream_kernel<false, true, false>", "tgemm_stream_kernel<false, false, true>",
     "tgemm_stream_kernel<false, true, true>", "tgemm_stream_kernel<true, false, false>"]
    + ["tgemm_kernel<false, true, 256, false>", "tgemm_kernel<true, true, 256, false>"]
    + ["tgemm_kernel<false, false, %d, %s>" % (w, a) for w in (128, 256) for a in ("false", "true")]
    + ["conv_smallci_kernel<%d, %s>" % (n, s) for n in range(1, 9) for s in ("false", "true")]
    + ["conv_smallco_%s_kernel<%d>" % (d, n) for n in range(1, 5) for d in ("fwd", "dgrad")]
    + ["wgrad_smallci_kernel<%d>" % n for n in range(1, 9)])


def smallci_wgrad_slices(B, Co, L):
    """The slice rule of regnet_conv1x1_wgrad_smallci_f32, by hand: about 1024 workgroups, slices of at least 4096 points."""
    groups = B * ((Co + 15) // 16)
    return max(1, min((1024 + groups - 1) // groups, (L + 4095) // 4096))


def smallci_wgrad_slice_len(B, Co, L):
    S = smallci_wgrad_slices(B, Co, L)
    return ((L + S - 1) // S + 255) // 256 * 256
