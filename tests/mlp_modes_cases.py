"""The shapes at which the gather, fused-first-layer and pre-multiplied modes of ``mlp_gemm_kernel`` and the three
feature-propagation glue kernels of csrc/mlp.hip are tested: one table per kernel for tests/test_mlp_modes_reference_cpu.py
(does every table reach the edges it has to) and tests/test_gpu_mlp_modes.py (the kernels at these shapes).  No torch.

The tile constants below are what the edges are computed from; the CPU test reads the ``#define`` lines of csrc/mlp.hip and
fails when they differ, so a retuned tile cannot silently move a case off its edge.  ``*_tags`` derive a case's properties
from its shape -- never from a hand-written list.

mlp_gemm_kernel<1 / 2 / 3> (``SA``; P = B * M * group rows, one 128 x 128 tile per workgroup, k-tiles of 16):
    interior_wide       P % 128 == 0, N % 128 == 0, ldc % 4 == 0: the LDS-transposed dwordx4 store (not pooled)
    interior_narrow     the same with ldc = N + 1: the unguarded dword store
    edge_rows           P % 128 != 0: the guarded store;  edge_rows_lt64: the last tile holds fewer than 64 rows
    edge_cols_1 / edge_cols_130     N = 1 / N = 130
    scene_boundary_in_tile          rows_per_scene % 128 != 0 with B >= 3: a tile's rows belong to two scenes
    group_16 / group_1  neighbourhood sizes other than 64 (the centre / V row of a tile's rows changes inside the tile)
    row0_redirect       a ragged last tile (its rows >= P read row 0's neighbour) with nbr[0] = Nsrc - 1
    index_extremes      neighbours and centres at 0 and Nsrc - 1, and ball-query style repeats of slot 0
    pool_single         pooled, P % 128 == 64: the last tile holds one neighbourhood (modes 2 and 3)
    pool_0 / pool_64
  mode 1: no_feat (Cf = 0, feat NULL); scalar_feat_cfirst (a channels-first strided view), scalar_feat_offset (channels-last,
    base pointer one float past a 16-byte boundary), scalar_feat_cf_mod4 (Cf % 4 != 0); vec_feat_4 / _16 / _256
    (channels-last, aligned: float4 loads); xyz_fills_ktile (Cf = 13), xyz_straddles_ktile_14 / _15, xyz_starts_ktile
    (Cf = 16); zero_ktile (Kpad one tile beyond ceil16(Cf + 3)); vec_twin (run a second time through the scalar path)
  mode 2: Cf_0 / Cf_3 / Cf_5, C1_16 / C1_128 / C1_256 (256 fills the LDS table of layer 1)
  mode 3: C1_4 / C1_20 (ragged last k-tile) / C1_128 / C1_256 / C1_512, Nsrc_1, B_3 (the V row is the global centre index)
``relu`` is the float test's setting; the exact test runs the other one.  ldc = N + ldc_pad (4 or 1).

interp_concat_kernel (``IC``; 4 rows per block, threads walk Cout in steps of 256), interp_affine_kernel (``IA``;
4 * 256 / (C / 4) rows per block) and score_head_kernel (``SH``; one wave per row, 4 rows per block): see the tag
functions.  ``special`` rows, counted from the last row backwards: zero_one (d2 = 0 in one slot: the eps clamp), zero_all
(in all three), dup (j0 = j1 = j2).
"""
import collections

BM = 128
BN = 128
BK = 16
IC_ROWS = 4
GLUE_THREADS = 256


def ceil_to(x, m):
    return (x + m - 1) // m * m


# ---- mlp_gemm_kernel<1 / 2 / 3> ---------------------------------------------------------------------------------------
# feat: "none" | "cfirst" | "offset" | "clast" (mode 1; mode 2 takes a channels-first view when Cf > 0);
# kx: extra k-tiles of Kpad (mode 1); opts: "extremes", "row0_last", "twin"
Sa = collections.namedtuple("Sa", "id mode B M group Nsrc N Cf C1 feat kx pool relu ldc_pad opts")


def _sa(id, mode, B, M, group, Nsrc, N, Cf=0, C1=0, feat="none", kx=0, pool=0, relu=1, ldc_pad=4, opts=()):
    return Sa(id, mode, B, M, group, Nsrc, N, Cf, C1, feat, kx, pool, relu, ldc_pad, frozenset(opts))


SA_CASES = [
    # ---- mode 1: gather
    _sa("g1-wide-vec16-starts", 1, 2, 2, 64, 37, 128, Cf=16, feat="clast", relu=1, ldc_pad=4),
    _sa("g1-narrow-nofeat", 1, 1, 2, 64, 37, 128, Cf=0, relu=0, ldc_pad=1),
    _sa("g1-scene-cfirst3-N130", 1, 3, 5, 16, 23, 130, Cf=3, feat="cfirst", relu=1, ldc_pad=4, opts=("extremes",)),
    _sa("g1-lt64-offset12-N1-g1", 1, 1, 150, 1, 11, 1, Cf=12, feat="offset", relu=0, ldc_pad=1, opts=("row0_last",)),
    _sa("g1-cf13-fills", 1, 1, 3, 64, 14, 128, Cf=13, feat="clast", relu=0, ldc_pad=4),
    _sa("g1-cf14-mod4", 1, 2, 3, 16, 9, 130, Cf=14, feat="clast", relu=1, ldc_pad=1),
    _sa("g1-cf15-cfirst-N1", 1, 3, 5, 16, 9, 1, Cf=15, feat="cfirst", relu=0, ldc_pad=4, opts=("extremes", "row0_last")),
    _sa("g1-vec4-zero-ktile", 1, 2, 1, 64, 5, 256, Cf=4, feat="clast", kx=1, relu=0, ldc_pad=4),
    _sa("g1-vec256-twin", 1, 3, 1, 64, 20, 128, Cf=256, feat="clast", relu=1, ldc_pad=4, opts=("twin",)),
    # ---- mode 2: layer 1 on the VALU inside the operand load
    _sa("f2-cf3-c128-pool-single", 2, 3, 1, 64, 30, 128, Cf=3, C1=128, feat="cfirst", pool=64, relu=1, ldc_pad=4),
    _sa("f2-cf0-c16-scene-N130", 2, 3, 5, 16, 23, 130, Cf=0, C1=16, relu=0, ldc_pad=1, opts=("extremes",)),
    _sa("f2-cf5-c256-wide", 2, 2, 2, 64, 40, 128, Cf=5, C1=256, feat="cfirst", relu=1, ldc_pad=4),
    _sa("f2-cf3-c256-pool-N130", 2, 2, 2, 64, 40, 130, Cf=3, C1=256, feat="cfirst", pool=64, relu=0, ldc_pad=1),
    _sa("f2-cf5-c128-narrow", 2, 1, 2, 64, 19, 128, Cf=5, C1=128, feat="cfirst", relu=0, ldc_pad=1),
    _sa("f2-lt64-c16-N1-g1", 2, 1, 150, 1, 11, 1, Cf=3, C1=16, feat="cfirst", relu=1, ldc_pad=4, opts=("row0_last",)),
    # ---- mode 3: relu(U[nbr] - V[centre]) operand
    _sa("p3-c4-lt64-N1-g1", 3, 1, 150, 1, 7, 1, C1=4, relu=1, ldc_pad=1, opts=("row0_last",)),
    _sa("p3-c20-scene-N130", 3, 3, 5, 16, 9, 130, C1=20, relu=0, ldc_pad=4, opts=("extremes",)),
    _sa("p3-c128-wide", 3, 2, 2, 64, 50, 128, C1=128, relu=1, ldc_pad=4),
    _sa("p3-c256-pool-single-N130", 3, 3, 1, 64, 33, 130, C1=256, pool=64, relu=0, ldc_pad=1),
    _sa("p3-c512-narrow", 3, 1, 2, 64, 21, 128, C1=512, relu=0, ldc_pad=1),
    _sa("p3-c128-nsrc1-pool", 3, 3, 2, 64, 1, 128, C1=128, pool=64, relu=1, ldc_pad=4),
]


def sa_rows(c):
    return c.B * c.M * c.group


def sa_kpad(c):
    """Kpad of the layer the MFMA loop runs: mode 1 ceil16(Cf + 3) (+ extra tiles), mode 2 C1, mode 3 ceil16(C1)."""
    if c.mode == 1:
        return ceil_to(c.Cf + 3, BK) + c.kx * BK
    return ceil_to(c.C1, BK)


def sa_tags(c):
    P, out = sa_rows(c), set()
    interior = P % BM == 0 and c.N % BN == 0 and not c.pool
    if interior and (c.N + c.ldc_pad) % 4 == 0:
        out.add("interior_wide")
    if interior and c.ldc_pad == 1:
        out.add("interior_narrow")
    if P % BM:
        out.add("edge_rows")
        if P % BM < 64:
            out.add("edge_rows_lt64")
        if "row0_last" in c.opts:
            out.add("row0_redirect")
    if c.N in (1, 130):
        out.add("edge_cols_%d" % c.N)
    if (c.M * c.group) % BM and c.B >= 3:
        out.add("scene_boundary_in_tile")
    if c.group != 64:
        out.add("group_%d" % c.group)
    if "extremes" in c.opts:
        out.add("index_extremes")
    out.add("pool_%d" % c.pool)
    if c.pool and P % BM == 64:
        out.add("pool_single")
    out.add("relu_%d" % c.relu)
    if c.mode == 1:
        if c.Cf == 0:
            out.add("no_feat")
        elif c.feat == "cfirst":
            out.add("scalar_feat_cfirst")
        elif c.feat == "offset" and c.Cf % 4 == 0:   # only the pointer keeps it off the float4 path
            out.add("scalar_feat_offset")
        elif c.Cf % 4:
            out.add("scalar_feat_cf_mod4")
        else:
            out.add("vec_feat_%d" % c.Cf)
            if "twin" in c.opts:
                out.add("vec_twin")
        if c.Cf % BK == 13:
            out.add("xyz_fills_ktile")
        if c.Cf % BK in (14, 15):
            out.add("xyz_straddles_ktile_%d" % (c.Cf % BK))
        if c.Cf and c.Cf % BK == 0:
            out.add("xyz_starts_ktile")
        if c.kx:
            out.add("zero_ktile")
    if c.mode == 2:
        out.update(("Cf_%d" % c.Cf, "C1_%d" % c.C1))
    if c.mode == 3:
        out.add("C1_%d" % c.C1)
        if c.Nsrc == 1:
            out.add("Nsrc_1")
        if c.B >= 3:
            out.add("B_3")
    return out


_SA_COMMON = {"interior_wide", "interior_narrow", "edge_rows", "edge_rows_lt64", "edge_cols_1", "edge_cols_130",
              "scene_boundary_in_tile", "group_16", "group_1", "row0_redirect", "index_extremes", "relu_0", "relu_1"}
SA_REQUIRED = {
    1: _SA_COMMON | {"no_feat", "scalar_feat_cfirst", "scalar_feat_offset", "scalar_feat_cf_mod4", "vec_feat_4", "vec_feat_16",
                     "vec_feat_256", "xyz_fills_ktile", "xyz_straddles_ktile_14", "xyz_straddles_ktile_15", "xyz_starts_ktile",
                     "zero_ktile", "vec_twin"},
    2: _SA_COMMON | {"pool_single", "pool_0", "pool_64", "Cf_0", "Cf_3", "Cf_5", "C1_16", "C1_128", "C1_256"},
    3: _SA_COMMON | {"pool_single", "pool_0", "pool_64", "C1_4", "C1_20", "C1_128", "C1_256", "C1_512", "Nsrc_1", "B_3"},
}

# ---- interp_concat_kernel ------------------------------------------------------------------------------------------------
# dense: "none" | "view" (channels 3.. of a wider channels-last buffer) | "cfirst" (contiguous (B, Cd, Nd)); ldo = Cout + ldo_pad
Ic = collections.namedtuple("Ic", "id B Nd Ns Cs Cd Cout ldo_pad dense special")
IC_CASES = [
    Ic("ic-P1-Ns1-cs4", 1, 1, 1, 4, 0, 8, 3, "none", ()),
    Ic("ic-P5-cs64-cd3", 1, 5, 6, 64, 3, 68, 1, "view", ("zero_one", "dup")),
    Ic("ic-P9-scene-cs300-cd5", 3, 3, 4, 300, 5, 308, 4, "cfirst", ("zero_all", "zero_one", "dup")),
    Ic("ic-P8-cs64-cd3-nopad", 2, 4, 5, 64, 3, 67, 2, "view", ("zero_one",)),
]


def ic_tags(c):
    P, out = c.B * c.Nd, {"Cs_%d" % c.Cs, "Cd_%d" % c.Cd}
    if c.Cout > c.Cs + c.Cd:
        out.add("pad_columns")
    if c.ldo_pad:
        out.add("sentinel_columns")
    if c.Cout > GLUE_THREADS:
        out.add("second_trip")
    if P in (1, 5):
        out.add("P_%d" % P)
    if P % IC_ROWS == 0:
        out.add("P_multiple_of_block")
    if P == 9 and c.Nd == 3:
        out.add("scene_boundary_in_block")
    if c.dense == "view":
        out.add("dense_view")
    if c.Ns == 1:
        out.update(("Ns_1", "dup"))
    out.update(c.special[:P])
    return out


IC_REQUIRED = {"Cs_4", "Cs_64", "Cs_300", "Cd_0", "Cd_3", "Cd_5", "pad_columns", "sentinel_columns", "second_trip", "P_1", "P_5",
               "P_multiple_of_block", "scene_boundary_in_block", "dense_view", "Ns_1", "zero_one", "zero_all", "dup"}

# ---- interp_affine_kernel ------------------------------------------------------------------------------------------------
# yd: 1 = a (P, C + 4) Yd operand; Cds: channels of the narrow skip input (0 = none), a strided view; relu as for SA
Ia = collections.namedtuple("Ia", "id B Nd Ns C yd Cds relu special")
IA_CASES = [
    Ia("ia-c4-P1", 1, 1, 1, 4, 0, 0, 1, ()),
    Ia("ia-c4-P1025", 1, 1025, 40, 4, 1, 2, 0, ("zero_one", "zero_all", "dup")),
    Ia("ia-c8-scene", 3, 5, 4, 8, 1, 3, 1, ("zero_one", "dup")),
    Ia("ia-c64-P63", 1, 63, 10, 64, 1, 0, 0, ("zero_all",)),
    Ia("ia-c64-P65", 5, 13, 6, 64, 0, 4, 1, ("zero_one",)),
    Ia("ia-c256-P40", 2, 20, 7, 256, 0, 0, 0, ("dup",)),
    Ia("ia-c512-scene", 3, 5, 4, 512, 1, 3, 1, ("zero_one", "zero_all", "dup")),
    Ia("ia-c1024-P3", 1, 3, 5, 1024, 0, 1, 0, ("zero_one",)),
    Ia("ia-c1024-P5", 1, 5, 5, 1024, 1, 2, 1, ("dup",)),
]


def ia_rows_per_block(C):
    return IC_ROWS * (GLUE_THREADS // (C // 4))


def ia_tags(c):
    P, rpb, out = c.B * c.Nd, ia_rows_per_block(c.C), {"C_%d" % c.C, "yd%d_small%d" % (c.yd, int(c.Cds > 0)), "relu_%d" % c.relu}
    if P == 1:
        out.add("P_1")
    if P == rpb - 1:
        out.add("block_minus_1_C%d" % c.C)
    if P == rpb + 1:
        out.add("block_plus_1_C%d" % c.C)
    if c.B >= 3 and c.Nd == 5 and rpb > c.Nd:
        out.add("scene_boundary_in_block")
    if c.Cds:
        out.add("Cd_small_%d" % c.Cds)
    if c.Ns == 1:
        out.add("dup")
    out.update(c.special[:P])
    return out


IA_REQUIRED = {"C_4", "C_8", "C_64", "C_256", "C_512", "C_1024", "P_1", "block_minus_1_C64", "block_plus_1_C64",
               "block_minus_1_C1024", "block_plus_1_C1024", "block_plus_1_C4", "scene_boundary_in_block", "yd0_small0", "yd0_small1",
               "yd1_small0", "yd1_small1", "Cd_small_1", "Cd_small_2", "Cd_small_3", "Cd_small_4", "relu_0", "relu_1", "zero_one",
               "zero_all", "dup"}
IA_REFUSALS = [(6, -1), (12, -3)]   # C -> REGNET_ERR_SHAPE (C % 4), REGNET_ERR_UNSUPPORTED (C / 4 does not divide 256)

# ---- score_head_kernel -----------------------------------------------------------------------------------------------------
# ldx = C + 3 with NaN padding.  Rows from the last one backwards, while the row index stays >= 1: v = 0 (score exactly 0.5),
# v ~ +100, v ~ -100 (expf overflows on one side)
Sh = collections.namedtuple("Sh", "id P C")
SH_CASES = [Sh("sh-P1-C1", 1, 1), Sh("sh-P3-C63", 3, 63), Sh("sh-P4-C64", 4, 64), Sh("sh-P5-C65", 5, 65), Sh("sh-P513-C200", 513, 200)]
SH_SPECIAL = ("v_zero", "v_plus_100", "v_minus_100")


def sh_tags(c):
    return {"C_%d" % c.C, "P_%d" % c.P} | set(SH_SPECIAL[:max(c.P - 1, 0)])


SH_REQUIRED = {"C_1", "C_63", "C_64", "C_65", "C_200", "P_1", "P_3", "P_4", "P_5", "P_513"} | set(SH_SPECIAL)
