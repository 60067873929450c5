"""The gather (mlp_gemm_kernel<1>), fused-first-layer (<2>) and pre-multiplied (<3>) layers and the feature-propagation glue
kernels of csrc/mlp.hip (interp_concat, interp_affine, score_head) on the MI355X, against the float64 restatements of
tests/mlp_modes_reference.py at the shapes of tests/mlp_modes_cases.py (which tests/test_mlp_modes_reference_cpu.py holds
against the edges they are there for).

The entry points are called with raw pointers so that every stride, padding and flag is the test's own:
  * operands with a leading dimension of their own (U, V, Yd: C + 4; x of the score head: C + 3) hold NaN in the padding;
  * W is packed [ceil128(N)][Kpad], zero padded; W1 [C1][8] and Wd4 [C][4] likewise;
  * every output has padding columns and eight extra rows prefilled with a sentinel that must survive the call.

exact   integers (mlp_modes_reference: A side in [-3, 3], W in [-2, 2], scale in {-1, 0.5, 1, 2}, integer shifts, interpolation
        weights 1/4, 1/4, 1/2): every intermediate is a multiple of 1/4 below 2^22, so ``torch.equal`` with the float64 reference
        cast to fp32 catches any dropped, duplicated or misplaced term, row, scene or column.  (Rows with d2 = 0 in all
        three slots have weights 1/3 and exist in the float test only; the score head has no exact mode beyond its v = 0 rows.)
float   random inputs scaled like the plain-layer test: |got - ref| <= tol elementwise with the derived bounds, finite outputs.
        ``pytest -s`` prints the worst error / tol of every case; REGNET_MLP_MODES_RECORD=<file> writes the maxima per kernel
        (profiles/mlp_mode_tests.txt).
Both call twice into fresh buffers and require equal bits.
"""
import collections
import os

import pytest
import torch

from . import gemm_reference as gref
from . import mlp_modes_cases as cases
from . import mlp_modes_reference as ref
from .test_gpu_gemm2_tiles import describe_mismatch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENT = -12345.0
EXTRA_ROWS = 8
OK, ERR_SHAPE, ERR_UNSUPPORTED = 0, -1, -3
SA_ENTRY = {1: "sa_layer1", 2: "sa_layer12", 3: "sa_premul_layer"}

_worst = collections.defaultdict(float)   # kernel -> largest error / tol seen by the float tests


@pytest.fixture(scope="module", autouse=True)
def record():
    yield
    path = os.environ.get("REGNET_MLP_MODES_RECORD")
    if path and _worst:
        with open(path, "w") as f:
            for kernel in sorted(_worst):
                f.write("%s %.4f\n" % (kernel, _worst[kernel]))


def _ids(table):
    return [c.id for c in table]


def _seed(table, c, base):
    return base + _ids(table).index(c.id)


def new_output(rows, cols, pad):
    return torch.full((rows + EXTRA_ROWS, cols + pad), SENT, device=DEV)


def check_sentinels(C, rows, cols, what):
    assert bool((C[:rows, cols:] == SENT).all()), "%s: a padding column of the output was written" % what
    assert bool((C[rows:] == SENT).all()), "%s: a row beyond the output was written" % what


def check_exact(run, want, what):
    rows, cols = want.shape
    C = run()
    check_sentinels(C, rows, cols, what)
    got, want = C[:rows, :cols], want.float()
    assert torch.equal(got, want), "%s: %s" % (what, describe_mismatch(got, want))
    assert torch.equal(run(), C), "%s: two calls differ" % what


def check_float(run, want, tol, what, kernel):
    rows, cols = want.shape
    C = run()
    check_sentinels(C, rows, cols, what)
    err = (C[:rows, :cols].double() - want).abs()
    assert bool(torch.isfinite(err).all()), "%s: non-finite output" % what
    # (columns that are copies have tol == 0 and must have err == 0: they count as ratio 0 or inf)
    ratio = float(torch.where(err > 0, err / tol, torch.zeros_like(err)).max())
    print("%s (%s): max error / tol = %.4f, max error %.3e" % (what, kernel, ratio, float(err.max())))
    _worst[kernel] = max(_worst[kernel], ratio)
    assert bool((err <= tol).all()), "%s: error / tol = %.3f" % (what, ratio)
    assert torch.equal(run(), C), "%s: two calls differ" % what
    return C


# ---- mlp_gemm_kernel<1 / 2 / 3> -------------------------------------------------------------------------------------------
def run_sa(c, d, relu, feat=None):
    """One call of the case's entry point into a fresh sentinel-filled buffer -> the whole buffer.  ``feat``: another
    (B, Nsrc, Cf) view to read the features from (mode 1)."""
    from regnet_for_3d_grasping_amd import _lib
    P, Kpad = cases.sa_rows(c), cases.sa_kpad(c)
    Wp = gref.pack_weight(d["w"], Kpad)
    C = new_output(P // 64 if c.pool else P, c.N, c.ldc_pad)
    xyz, nbr, ctr = d["xyz"], d["nbr"], d["ctr"]
    assert nbr.is_contiguous() and ctr.is_contiguous() and Wp.shape[0] % 128 == 0
    assert int(nbr.min()) >= 0 and int(nbr.max()) < c.Nsrc and int(ctr.min()) >= 0 and int(ctr.max()) < c.Nsrc
    out = (Wp.data_ptr(), Kpad, d["scale"].data_ptr(), d["shift"].data_ptr(), C.data_ptr(), C.stride(0), c.N, relu)
    if c.mode == 3:
        U, V = d["U"], d["V"]
        assert U.stride(0) == c.C1 + 4 and V.stride(0) == c.C1 + 4 and tuple(U.shape) == (c.B * c.Nsrc, c.C1 + 4)
        _lib.call("regnet_sa_premul_layer_f32", U, U.data_ptr(), U.stride(0), V.data_ptr(), V.stride(0), c.C1, nbr.data_ptr(),
                  c.B, c.Nsrc, c.M, c.group, *out, c.pool)
        return C
    feat = d["feat"] if feat is None else feat
    if c.Cf:
        assert tuple(feat.shape) == (c.B, c.Nsrc, c.Cf)
        fargs = (feat.data_ptr(), feat.stride(0), feat.stride(1), feat.stride(2), c.Cf)
    else:
        fargs = (None, 0, 0, 0, 0)
    gather = fargs + (xyz.data_ptr(),) + tuple(xyz.stride()) + (nbr.data_ptr(), ctr.data_ptr(), c.B, c.M, c.group)
    if c.mode == 1:
        _lib.call("regnet_sa_layer1_f32", xyz, *gather, *out)
    else:
        W8 = d["W8"]
        assert tuple(W8.shape) == (c.C1, 8) and W8.is_contiguous() and Kpad == c.C1
        _lib.call("regnet_sa_layer12_f32", xyz, *gather, W8.data_ptr(), d["scale1"].data_ptr(), d["shift1"].data_ptr(), c.C1,
                  *out, c.pool)
    return C


@pytest.mark.parametrize("c", cases.SA_CASES, ids=_ids(cases.SA_CASES))
def test_sa_exact_integers(c):
    relu = 1 - c.relu
    d = ref.sa_inputs(c, True, _seed(cases.SA_CASES, c, 1000), DEV)
    want, _, parts = ref.sa_reference(c, d, relu, cases.sa_kpad(c))
    assert max(float(t.abs().max()) for t in parts) < 2 ** 22
    check_exact(lambda: run_sa(c, d, relu), want, c.id)


@pytest.mark.parametrize("c", cases.SA_CASES, ids=_ids(cases.SA_CASES))
def test_sa_float_within_derived_bound(c):
    d = ref.sa_inputs(c, False, _seed(cases.SA_CASES, c, 2000), DEV)
    want, tol, _ = ref.sa_reference(c, d, c.relu, cases.sa_kpad(c))
    C = check_float(lambda: run_sa(c, d, c.relu), want, tol, c.id, SA_ENTRY[c.mode])
    if "twin" in c.opts:
        # the same values in a channels-first buffer: the scalar feature loads build the same operand, bit for bit
        twin = ref.feat_layout(d["feat"], "cfirst")
        assert d["feat"].stride(2) == 1 and twin.stride(2) != 1 and torch.equal(twin, d["feat"])
        assert torch.equal(run_sa(c, d, c.relu, feat=twin), C), "%s: the float4 and the scalar feature loads differ" % c.id


# ---- interp_concat_kernel --------------------------------------------------------------------------------------------------
def run_ic(c, d):
    from regnet_for_3d_grasping_amd import _lib
    sparse, idx, dist2, dense = d["sparse"], d["idx"], d["dist2"], d["dense"]
    out = new_output(c.B * c.Nd, c.Cout, c.ldo_pad)
    assert sparse.is_contiguous() and idx.is_contiguous() and dist2.is_contiguous()
    assert int(idx.min()) >= 0 and int(idx.max()) < c.Ns
    dargs = (None, 0, 0, 0) if dense is None else (dense.data_ptr(),) + tuple(dense.stride())
    _lib.call("regnet_interp_concat_f32", sparse, sparse.data_ptr(), sparse.stride(0), sparse.stride(1), c.Cs, idx.data_ptr(),
              dist2.data_ptr(), d["eps"], *dargs, c.Cd, c.B, c.Nd, out.data_ptr(), out.stride(0), c.Cout)
    return out


@pytest.mark.parametrize("c", cases.IC_CASES, ids=_ids(cases.IC_CASES))
@pytest.mark.parametrize("exact", [True, False], ids=["exact", "float"])
def test_interp_concat(c, exact):
    d = ref.ic_inputs(c, exact, _seed(cases.IC_CASES, c, 3000 + exact), DEV)
    want, tol, _ = ref.interp_concat(d["sparse"], d["idx"], d["dist2"], d["eps"], d["dense"], c.Cout)
    if exact:
        check_exact(lambda: run_ic(c, d), want, c.id)
    else:
        # (the dense and the zero pad columns have tol == 0: copies, bit for bit)
        check_float(lambda: run_ic(c, d), want, tol, c.id, "interp_concat")


# ---- interp_affine_kernel --------------------------------------------------------------------------------------------------
def run_ia(c, d, relu, C=None, tolerate=0):
    from regnet_for_3d_grasping_amd import _lib
    C = c.C if C is None else C
    ys, idx, dist2, yd, ds, wd4 = d["ys"], d["idx"], d["dist2"], d["yd"], d["dense_small"], d["wd4"]
    out = new_output(c.B * c.Nd, c.C, 4)
    assert ys.is_contiguous() and idx.is_contiguous() and dist2.is_contiguous() and int(idx.min()) >= 0 and int(idx.max()) < c.Ns
    assert yd is None or (yd.stride(0) == c.C + 4 and yd.shape[0] == c.B * c.Nd)
    dargs = (None, 0, 0, 0, 0, None) if ds is None else (ds.data_ptr(),) + tuple(ds.stride()) + (c.Cds, wd4.data_ptr())
    rc = _lib.call("regnet_interp_affine_f32", ys, ys.data_ptr(), ys.stride(0), ys.stride(1), idx.data_ptr(), dist2.data_ptr(),
                   d["eps"], None if yd is None else yd.data_ptr(), 0 if yd is None else yd.stride(0), *dargs,
                   d["scale"].data_ptr(), d["shift"].data_ptr(), relu, c.B, c.Nd, C, out.data_ptr(), out.stride(0),
                   tolerate=tolerate)
    return out, rc


def _ia_reference(d, relu):
    return ref.interp_affine(d["ys"], d["idx"], d["dist2"], d["eps"], d["yd"], d["dense_small"], d["wd4"], d["scale"], d["shift"],
                             relu)


@pytest.mark.parametrize("c", cases.IA_CASES, ids=_ids(cases.IA_CASES))
def test_interp_affine_exact_integers(c):
    relu = 1 - c.relu
    d = ref.ia_inputs(c, True, _seed(cases.IA_CASES, c, 4000), DEV)
    check_exact(lambda: run_ia(c, d, relu)[0], _ia_reference(d, relu)[0], c.id)


@pytest.mark.parametrize("c", cases.IA_CASES, ids=_ids(cases.IA_CASES))
def test_interp_affine_float_within_derived_bound(c):
    d = ref.ia_inputs(c, False, _seed(cases.IA_CASES, c, 5000), DEV)
    want, tol, _ = _ia_reference(d, c.relu)
    check_float(lambda: run_ia(c, d, c.relu)[0], want, tol, c.id, "interp_affine")


@pytest.mark.parametrize("C,status", cases.IA_REFUSALS)
def test_interp_affine_refuses_row_widths_it_cannot_walk(C, status):
    """C % 4 != 0 is a shape error, C / 4 not dividing 256 unsupported; nothing is launched (the buffers are those of a
    C = 64 case, so even a launch would stay inside them)."""
    c = cases.Ia("refusal", 2, 5, 4, 64, 1, 3, 1, ())
    d = ref.ia_inputs(c, False, 6000, DEV)
    out, rc = run_ia(c, d, 1, C=C, tolerate=status)
    torch.cuda.synchronize()
    assert rc == status and status in (ERR_SHAPE, ERR_UNSUPPORTED)
    assert bool((out == SENT).all())
    with pytest.raises(RuntimeError):
        run_ia(c, d, 1, C=C)


# ---- score_head_kernel -----------------------------------------------------------------------------------------------------
def run_sh(c, d):
    from regnet_for_3d_grasping_amd import _lib
    x, w = d["x"], d["w"]
    out = new_output(c.P, 1, 0)
    assert x.stride(0) == c.C + 3 and w.is_contiguous()
    _lib.call("regnet_score_head_f32", x, x.data_ptr(), x.stride(0), c.C, w.data_ptr(), ref.SH_BIAS, ref.SH_SCALE, ref.SH_SHIFT,
              out.data_ptr(), c.P)
    return out


@pytest.mark.parametrize("c", cases.SH_CASES, ids=_ids(cases.SH_CASES))
def test_score_head_within_derived_bound(c):
    d = ref.sh_inputs(c, cases.SH_SPECIAL, _seed(cases.SH_CASES, c, 7000), DEV)
    score, tol, (v, _) = ref.score_head(d["x"], c.C, d["w"], ref.SH_BIAS, ref.SH_SCALE, ref.SH_SHIFT)
    C = check_float(lambda: run_sh(c, d), score.view(-1, 1), tol.view(-1, 1), c.id, "score_head")
    rows = d["rows"]
    assert set(rows) == cases.sh_tags(c) & set(cases.SH_SPECIAL)
    if "v_zero" in rows:
        assert float(v[rows["v_zero"]]) == 0.0 and float(C[rows["v_zero"], 0]) == 0.5
    for kind in ("v_plus_100", "v_minus_100"):
        if kind in rows:   # expf(-v) overflows for v ~ -100 and underflows for v ~ +100: finite (check_float) and in [0, 1]
            assert abs(float(v[rows[kind]])) > 99 and 0.0 <= float(C[rows[kind], 0]) <= 1.0
