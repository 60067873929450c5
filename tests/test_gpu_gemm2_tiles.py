"""The plain-layer GEMM (csrc/gemm2.h behind regnet_mlp_layer_f32, csrc/mlp.hip) on the MI355X at every tile configuration of its
dispatch, against the float64 restatement of the layer (tests/gemm_reference.py).  The shapes are the table of
tests/gemm2_cases.py, which tests/test_gemm2_plan_cpu.py holds against the library's own plan: configurations D / C / E with
and without a split tail, a tail slice that starts beyond P, ragged last column tiles, the pooled epilogue of the large
tiles, full and open slabs of K, the small tile A at its edges and the two-buffer kernel M at Kpad == 16.

The entry point is called with raw pointers so that lda, Ka, ldc, relu and pool_group are the test's own:
  * A has lda = Ka + 4 and NaN in the columns >= Ka (the header: never read into a product);
  * W is packed [ceil128(N)][Kpad], zero padded;
  * C has ldc = N + 4 or N + 1, eight extra rows, and is prefilled with a sentinel: every padding column and extra row must
    still hold it after the call -- an out-of-range store of a ragged tile or tail slice lands there, not in unowned memory.

exact   integers: A in [-3, 3], W in [-2, 2], scale in {-1, 0.5, 1, 2}, integer shifts.  Every product and partial sum is an
        integer below 2^24, so any order of additions, slabbed or not, gives the same fp32 value: ``torch.equal`` with the
        float64 reference cast to fp32 catches any dropped, duplicated or misplaced k-term, row or column.
float   A = randn, W = randn / sqrt(K), scale in +-[0.5, 1.5], shift = 0.1 randn: |got - ref| <= tol elementwise with the
        derived bound of gemm_reference (nothing fitted).  ``pytest -s`` prints the worst error / tol of every case;
        REGNET_GEMM2_RECORD=<file> writes the maxima per configuration (profiles/gemm2_tile_tests.txt).
Both call twice into fresh buffers and require equal bits (determinism).
"""
import collections
import os

import pytest
import torch

from . import gemm2_cases as cases
from . import gemm_reference as ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENT = -12345.0
EXTRA_ROWS = 8
IDS = [c.id for c in cases.CASES]

_worst = collections.defaultdict(float)   # configuration -> largest error / tol seen by the float tests


@pytest.fixture(scope="module", autouse=True)
def record():
    yield
    path = os.environ.get("REGNET_GEMM2_RECORD")
    if path and _worst:
        with open(path, "w") as f:
            for config in sorted(_worst):
                f.write("%s %.4f\n" % (config, _worst[config]))


def make_inputs(N, K, P, exact, seed):
    """-> A (P, K + 4) with NaN beyond column K, w (N, K), scale (N), shift (N), all float32 on the device."""
    g = torch.Generator(device=DEV).manual_seed(seed)
    A = torch.full((P, K + 4), float("nan"), device=DEV)
    if exact:
        A[:, :K] = torch.randint(-3, 4, (P, K), generator=g, device=DEV).float()
        w = torch.randint(-2, 3, (N, K), generator=g, device=DEV).float()
        scale = torch.tensor([-1.0, 0.5, 1.0, 2.0], device=DEV)[torch.randint(0, 4, (N,), generator=g, device=DEV)]
        shift = torch.randint(-4, 5, (N,), generator=g, device=DEV).float()
    else:
        A[:, :K] = torch.randn(P, K, generator=g, device=DEV)
        w = torch.randn(N, K, generator=g, device=DEV) / K ** 0.5
        sign = torch.randint(0, 2, (N,), generator=g, device=DEV).float() * 2 - 1
        scale = sign * (torch.rand(N, generator=g, device=DEV) + 0.5)
        shift = torch.randn(N, generator=g, device=DEV) * 0.1
    return A, w, scale, shift


def new_output(rows, N, ldc_pad):
    return torch.full((rows + EXTRA_ROWS, N + ldc_pad), SENT, device=DEV)


def run_layer(A, K, Wp, scale, shift, P, N, relu, pool, ldc_pad):
    """One regnet_mlp_layer_f32 call into a fresh sentinel-filled buffer -> the whole buffer."""
    from regnet_for_3d_grasping_amd import _lib
    C = new_output(P // 64 if pool else P, N, ldc_pad)
    assert A.stride(0) == K + 4 and Wp.shape[0] % 128 == 0 and Wp.is_contiguous() and C.is_contiguous()
    _lib.call("regnet_mlp_layer_f32", A, A.data_ptr(), A.stride(0), K, Wp.data_ptr(), Wp.shape[1], scale.data_ptr(),
              shift.data_ptr(), C.data_ptr(), C.stride(0), P, N, relu, pool)
    return C


def run_splitk(A, K, Wp, scale, shift, P, N, relu, ksplit, ldc_pad):
    from regnet_for_3d_grasping_amd import _lib
    C = new_output(P, N, ldc_pad)
    nbytes = _lib.call("regnet_mlp_splitk_workspace_bytes", None, P, N, ksplit)
    ws = torch.full((nbytes // 4 + 64,), SENT, device=DEV)
    _lib.call("regnet_mlp_layer_splitk_f32", A, A.data_ptr(), A.stride(0), K, Wp.data_ptr(), Wp.shape[1], scale.data_ptr(),
              shift.data_ptr(), C.data_ptr(), C.stride(0), P, N, relu, ksplit, ws.data_ptr() if nbytes else None)
    assert bool((ws[nbytes // 4:] == SENT).all()), "a store beyond the split-K workspace"
    return C


def check_sentinels(C, rows, N, what):
    assert bool((C[:rows, N:] == SENT).all()), "%s: a padding column of C was written" % what
    assert bool((C[rows:] == SENT).all()), "%s: a row beyond the output was written" % what


def describe_mismatch(got, want):
    bad = (got != want).nonzero()
    r, c = bad[:, 0], bad[:, 1]
    return "%d of %d elements differ: rows %d..%d, columns %d..%d, first (%d, %d): got %r, want %r" % (
        bad.shape[0], got.numel(), int(r.min()), int(r.max()), int(c.min()), int(c.max()), int(r[0]), int(c[0]),
        float(got[r[0], c[0]]), float(want[r[0], c[0]]))


def check_exact(run, A, K, w, scale, shift, relu, pool, what):
    N = w.shape[0]
    want, S, _ = ref.reference(A, K, w, scale, shift, relu, pool)
    assert float(S.abs().max()) * 2 + 4 < 2 ** 24
    rows = want.shape[0]
    C = run()
    check_sentinels(C, rows, N, what)
    got = C[:rows, :N]
    want = want.float()
    assert torch.equal(got, want), "%s: %s" % (what, describe_mismatch(got, want))
    assert torch.equal(run(), C), "%s: two calls differ" % what


def check_float(run, A, K, Kpad, w, scale, shift, relu, pool, what, config):
    N = w.shape[0]
    want, S, T = ref.reference(A, K, w, scale, shift, relu, pool)
    tol = ref.tolerance(S, T, scale, shift, Kpad, pool)
    rows = want.shape[0]
    C = run()
    check_sentinels(C, rows, N, what)
    err = (C[:rows, :N].double() - want).abs()
    assert bool(torch.isfinite(err).all()), "%s: non-finite output" % what
    ratio = float((err / tol).max())
    print("%s (%s): max error / tol = %.4f, max error %.3e" % (what, config, ratio, float(err.max())))
    _worst[config] = max(_worst[config], ratio)
    assert bool((err <= tol).all()), "%s: error / tol = %.3f" % (what, ratio)
    assert torch.equal(run(), C), "%s: two calls differ" % what
    return C


def _layer_runner(case, A, w, scale, shift, relu):
    Wp = ref.pack_weight(w, cases.kpad(case))
    return lambda: run_layer(A, case.K, Wp, scale, shift, case.P, case.N, relu, case.pool, case.ldc_pad)


@pytest.mark.parametrize("case", cases.CASES, ids=IDS)
def test_exact_integers(case):
    assert cases.plan_of(case)["config"] == case.config
    relu = 1 - case.relu
    A, w, scale, shift = make_inputs(case.N, case.K, case.P, True, 1000 + IDS.index(case.id))
    check_exact(_layer_runner(case, A, w, scale, shift, relu), A, case.K, w, scale, shift, relu, case.pool, case.id)


@pytest.mark.parametrize("case", cases.CASES, ids=IDS)
def test_float_within_derived_bound(case):
    assert cases.plan_of(case)["config"] == case.config
    A, w, scale, shift = make_inputs(case.N, case.K, case.P, False, 2000 + IDS.index(case.id))
    check_float(_layer_runner(case, A, w, scale, shift, case.relu), A, case.K, cases.kpad(case), w, scale, shift, case.relu,
                case.pool, case.id, case.config)


@pytest.mark.parametrize("case", [c for c in cases.CASES if c.config == "C"], ids=[c for c in IDS if c.startswith("C-")])
def test_configuration_c_adds_in_the_order_of_configuration_a(case):
    """csrc/mlp.hip (plan_gemm2) says the two-per-CU 128 x 128 tile adds in the same order as the 64 x 128 tile: the first
    1000 rows of a C launch against the same rows as a P = 1000 launch (configuration A), bit for bit."""
    rows = 1000
    rc, plan = cases.query_plan(rows, case.N, cases.kpad(case), 0)
    assert rc == 0 and plan["config"] == "A" and cases.plan_of(case)["config"] == "C"
    A, w, scale, shift = make_inputs(case.N, case.K, case.P, False, 3000 + IDS.index(case.id))
    Wp = ref.pack_weight(w, cases.kpad(case))
    big = run_layer(A, case.K, Wp, scale, shift, case.P, case.N, case.relu, 0, case.ldc_pad)
    small = run_layer(A, case.K, Wp, scale, shift, rows, case.N, case.relu, 0, case.ldc_pad)
    check_sentinels(small, rows, case.N, case.id)
    got, want = big[:rows, :case.N], small[:rows, :case.N]
    assert torch.equal(got, want), describe_mismatch(got, want)


# regnet_mlp_layer_splitk_f32 directly: one slice (no workspace, no second kernel), the most slices (one k-tile each) and a
# slice count that does not divide the 33 k-tiles (slices of 7, the last one of 5) with a ragged N and unaligned C rows
SPLITK = [(70, 128, 516, 1, 4, 1), (70, 128, 516, 33, 4, 0), (70, 130, 516, 5, 1, 1)]   # P, N, K, ksplit, ldc_pad, float test's relu


@pytest.mark.parametrize("P,N,K,ksplit,ldc_pad,relu", SPLITK)
@pytest.mark.parametrize("exact", [True, False], ids=["exact", "float"])
def test_splitk_entry_point(P, N, K, ksplit, ldc_pad, relu, exact):
    Kpad = ref.ceil_to(K, 16)
    assert ksplit <= Kpad // 16 and (ksplit in (1, Kpad // 16) or N % 128)
    relu = 1 - relu if exact else relu
    A, w, scale, shift = make_inputs(N, K, P, exact, 4000 + ksplit)
    Wp = ref.pack_weight(w, Kpad)
    what = "split-K %d" % ksplit

    def run():
        return run_splitk(A, K, Wp, scale, shift, P, N, relu, ksplit, ldc_pad)
    if exact:
        check_exact(run, A, K, w, scale, shift, relu, 0, what)
    else:
        # the slices' partial sums are added by the second kernel: still one tree over Kpad products (gemm_reference)
        check_float(run, A, K, Kpad, w, scale, shift, relu, 0, what, "splitk")
