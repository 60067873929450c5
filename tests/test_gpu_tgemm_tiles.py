"""The training GEMM (csrc/tgemm.hip: forward, input gradient and weight gradient of the 1x1 convolutions, and the small-channel
kernels beside them) on the MI355X at every kernel edge, against a float64 restatement of the same contraction.  The shapes are
the table of tests/tgemm_cases.py, which tests/test_tgemm_plan_cpu.py holds against the library's host side.

Every call goes to the C entry point with raw pointers into buffers of the test's own:
  * every operand and output is 16-byte aligned inside a larger allocation, 64 elements of guard in front of it and behind it;
  * the guards of inputs hold NaN: a term read outside an operand poisons the output element it enters;
  * the guards of outputs, of the statistics and of the workspaces hold a sentinel that must still be there after the call,
    and so does the body of an output before the call (an element that is not written is seen);
  * the ticket is a fresh zeroed int32 per call.

exact   small integers: x in [-3, 3], W and dY in [-2, 2], affine scale in {-1, 0.5, 1, 2} with integer shifts.  Every product
        and partial sum is a half-integer below 2^23 (asserted on the reference: max |W| . |a| < 2^23), so any order of additions
        gives the same fp32 value: ``torch.equal`` with the float64 reference catches any dropped, doubled or misplaced k-tile,
        row, column, tile, slice or scene.  With statistics: x in [-2, 2], W in [-1, 1] (affine: scale +-1, shift and x in [-1, 1]):
        64 y^2 <= 2^24 (asserted), the fp32 partials of the sums are exact and so are the fp64 table and atomics: the sums must
        EQUAL the float64 sums of the reference, and Y must equal, bit for bit, the same call without statistics.
float   randn inputs, W / sqrt(K): |got - ref| <= gamma(n) T [+ u T with an affine operand: the one rounding of the fragment value],
        T = |W| . |a|, gamma and u of tests/gemm_reference.py, nothing fitted.  n counts the roundings a product can pass:
          forward / input gradient    K + 1          (its own, if the matrix unit rounds it, and K - 1 additions)
          weight gradient             L / S + B S    (the chain inside a slice, then the partial matrices in order)
          small Ci forward / small Co Ci resp. Co    (one fused multiply-add per term)
          small Ci weight gradient    9 + steps      (product, two in-step additions, steps = slice length / 256 accumulations,
                                                      six shuffle additions; the test adds the partial matrices in float64)
        The float64 reference evaluates the affine from the fp32 x, scale and shift.  The statistics are held against the float64
        sums of the kernel's own Y: at most 8 fp32 roundings (in-lane sum or squares, five halving steps) before the fp64 table.
        ``pytest -s`` prints the worst error / tol; REGNET_TGEMM_RECORD=<file> writes the maxima per kernel instantiation, the CU
        count and the grid / total of the persistent cases (profiles/tgemm_tile_tests.txt).
Both modes call twice into fresh buffers and require equal bits, and require the stream entry point and the one-workgroup-per-tile
entry point (forward and input gradient without affine or statistics) to give equal bits, as include/regnet_hip.h promises.

No shape here is one the launchers refuse, except in test_refusals, where the host refuses before any launch.
"""
import collections
import math
import os

import pytest
import torch

from . import gemm_reference as gref
from . import tgemm_cases as cases

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 64
SENT = -12345.0
OK = 0

_worst = collections.defaultdict(float)     # kernel instantiation -> largest error / tol of the float tests
_persistent = []                            # (what, grid, total) of the persistent cases


@pytest.fixture(scope="module", autouse=True)
def record():
    yield
    path = os.environ.get("REGNET_TGEMM_RECORD")
    if path and _worst:
        with open(path, "w") as f:
            f.write("# worst error / tol of tests/test_gpu_tgemm_tiles.py per kernel instantiation (all must be < 1)\n")
            f.write("compute units %d\n" % compute_units())
            for name in sorted(_worst):
                f.write("%-48s %.4f\n" % (name, _worst[name]))
            f.write("# persistent cases: grid and total output tiles\n")
            for what, grid, total in _persistent:
                f.write("%-48s grid %d total %d\n" % (what, grid, total))


def compute_units():
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


# ---------------------------------------------------------------------------------------------------------------- buffers
def guarded_input(t):
    """-> a copy of ``t`` (same shape) that is 16-byte aligned inside an allocation with GUARD NaNs in front of it and behind it."""
    n = t.numel()
    whole = torch.full((n + 2 * GUARD,), float("nan"), dtype=t.dtype, device=DEV)
    body = whole[GUARD:GUARD + n]
    body.copy_(t.reshape(-1))
    assert body.data_ptr() % 16 == 0
    return body.view(t.shape)


class Out:
    """An output of ``shape``: sentinel everywhere, GUARD elements in front of the body and behind it."""

    def __init__(self, shape, dtype=torch.float32):
        n = int(math.prod(shape))
        self.whole = torch.full((n + 2 * GUARD,), SENT, dtype=dtype, device=DEV)
        self.body = self.whole[GUARD:GUARD + n].view(shape)
        assert self.body.data_ptr() % 16 == 0

    def ptr(self, byte_offset=0):
        return self.body.data_ptr() + byte_offset

    def guards_intact(self):
        n = self.body.numel()
        return bool((self.whole[:GUARD] == SENT).all()) and bool((self.whole[GUARD + n:] == SENT).all())

    def untouched(self):
        return bool((self.whole == SENT).all())


def new_ticket():
    return torch.zeros(1, dtype=torch.int32, device=DEV)


# ----------------------------------------------------------------------------------------------------------------- inputs
def k_of(c):
    return c.Co if c.op == "dgrad" or (c.op == "smallco" and c.direction) else c.Ci


def make_inputs(c, mode, seed):
    """mode: "exact", "stats" (exact with the narrower ranges of the statistics) or "float" -> dict of guarded fp32 tensors:
    W (Co, Ci), X (B, Ci, L), dY (B, Co, L), scale / shift (Ci), bias (Co) -- those the operation reads."""
    g = torch.Generator(device=DEV).manual_seed(seed)

    def ints(shape, lo, hi):
        return torch.randint(lo, hi + 1, shape, generator=g, device=DEV).float()

    def randn(*shape):
        return torch.randn(*shape, generator=g, device=DEV)
    B = max(c.B, 1)
    takes_dy = c.op in ("dgrad", "wgrad", "wgrad_smallci") or (c.op == "smallco" and c.direction)
    takes_x = not (c.op == "dgrad" or (c.op == "smallco" and c.direction))
    takes_w = c.op not in ("wgrad", "wgrad_smallci")
    inp = {}
    if mode == "float":
        if takes_w:
            inp["W"] = randn(c.Co, c.Ci) / k_of(c) ** 0.5
        if takes_x:
            inp["X"] = randn(B, c.Ci, c.L)
        if takes_dy:
            inp["dY"] = randn(B, c.Co, c.L)
        if c.affine:
            sign = ints((c.Ci,), 0, 1) * 2 - 1
            inp["scale"] = sign * (torch.rand(c.Ci, generator=g, device=DEV) + 0.5)
            inp["shift"] = randn(c.Ci) * 0.1
        if c.bias:
            inp["bias"] = randn(c.Co)
    else:
        stats = mode == "stats"
        if takes_w:
            inp["W"] = ints((c.Co, c.Ci), -1, 1) if stats else ints((c.Co, c.Ci), -2, 2)
        if takes_x:
            r = (1 if c.affine else 2) if stats else 3
            inp["X"] = ints((B, c.Ci, c.L), -r, r)
        if takes_dy:
            inp["dY"] = ints((B, c.Co, c.L), -2, 2)
        if c.affine:
            if stats:
                inp["scale"] = ints((c.Ci,), 0, 1) * 2 - 1
                inp["shift"] = ints((c.Ci,), -1, 1)
            else:
                inp["scale"] = torch.tensor([-1.0, 0.5, 1.0, 2.0], device=DEV)[torch.randint(0, 4, (c.Ci,), generator=g, device=DEV)]
                inp["shift"] = ints((c.Ci,), -4, 4)
        if c.bias:
            inp["bias"] = ints((c.Co,), -4, 4)
    return {k: guarded_input(v) for k, v in inp.items()}


def reference(c, inp):
    """-> (result, T) in float64: the operation of ``c`` and the same with every factor's magnitude (T = |W| . |a|)."""
    B = c.B
    a = None
    if "X" in inp:
        a = inp["X"][:B].double()
        if c.affine:
            a = a * inp["scale"].double()[None, :, None] + inp["shift"].double()[None, :, None]
            if c.relu:
                a = a.clamp_min(0.0)
    if c.op in ("fwd", "smallci") or (c.op == "smallco" and not c.direction):
        w = inp["W"].double()
        y, T = w @ a, w.abs() @ a.abs()
        if c.bias:
            y = y + inp["bias"].double()[None, :, None]
            T = T + inp["bias"].double().abs()[None, :, None]
        return y, T
    if c.op in ("dgrad", "smallco"):
        w, dy = inp["W"].double().t(), inp["dY"][:B].double()
        return w @ dy, w.abs() @ dy.abs()
    dy = inp["dY"][:B].double()
    return (dy @ a.transpose(1, 2)).sum(0), (dy.abs() @ a.abs().transpose(1, 2)).sum(0)


def roundings(c):
    """n of the module docstring."""
    if c.op in ("fwd", "dgrad"):
        return k_of(c) + 1
    if c.op == "wgrad":
        S = wgrad_slices(c)
        return c.L // S + c.B * S
    if c.op in ("smallci", "smallco"):
        return k_of(c)
    return 9 + cases.smallci_wgrad_slice_len(c.B, c.Co, c.L) // 256


def wgrad_slices(c):
    from regnet_for_3d_grasping_amd import _lib
    S = int(_lib.call("regnet_conv1x1_wgrad_slices", None, c.B, c.Co, c.Ci, c.L))
    assert c.slices is None or S == c.slices
    return S


# ------------------------------------------------------------------------------------------------------------------ calls
Result = collections.namedtuple("Result", "rc out sums workspace")


def _p(inp, name):
    return inp[name].data_ptr()


def run(c, inp, entry="stream", stats=None, fault=None, tolerate=0):
    """One call of the entry point of ``c`` into fresh sentinel-filled buffers.  entry: "stream" or "tile" (forward and input
    gradient without affine or statistics only); stats: override of c.stats; fault: see tgemm_cases.REJECTS."""
    from regnet_for_3d_grasping_amd import _lib
    stats = c.stats if stats is None else stats
    B, Co, Ci, L = c.B, c.Co, c.Ci, c.L
    Bm = max(B, 1)
    anchor = next(iter(inp.values()))
    off = 4 if fault == "misaligned" else 0
    tick = None if fault == "null_ticket" else new_ticket()
    tp = None if tick is None else tick.data_ptr()
    sums = ws = None
    if c.op == "fwd":
        out = Out((Bm, Co, L))
        if stats:
            sums = Out((2 * Co,), torch.float64)
            rc = _lib.call("regnet_conv1x1_fwd_stats_stream_f32", anchor, _p(inp, "W"), _p(inp, "X"), out.ptr(off), B, Co, Ci, L,
                           _p(inp, "scale") if c.affine else None, _p(inp, "shift") if c.affine else None, c.relu, tp, sums.ptr(),
                           tolerate=tolerate)
        elif c.affine:
            rc = _lib.call("regnet_conv1x1_fwd_bnrelu_stream_f32", anchor, _p(inp, "W"), _p(inp, "X"), out.ptr(off), B, Co, Ci, L,
                           _p(inp, "scale"), _p(inp, "shift"), c.relu, tp, tolerate=tolerate)
        elif entry == "stream":
            rc = _lib.call("regnet_conv1x1_fwd_stream_f32", anchor, _p(inp, "W"), _p(inp, "X"), out.ptr(off), B, Co, Ci, L, tp,
                           tolerate=tolerate)
        else:
            rc = _lib.call("regnet_conv1x1_fwd_f32", anchor, _p(inp, "W"), _p(inp, "X"), out.ptr(off), B, Co, Ci, L, tolerate=tolerate)
    elif c.op == "dgrad":
        out = Out((Bm, Ci, L))
        if entry == "stream":
            rc = _lib.call("regnet_conv1x1_dgrad_stream_f32", anchor, _p(inp, "W"), _p(inp, "dY"), out.ptr(off), B, Co, Ci, L, tp,
                           tolerate=tolerate)
        else:
            rc = _lib.call("regnet_conv1x1_dgrad_f32", anchor, _p(inp, "W"), _p(inp, "dY"), out.ptr(off), B, Co, Ci, L, tolerate=tolerate)
    elif c.op == "wgrad":
        out = Out((Co, Ci))
        nbytes = int(_lib.call("regnet_conv1x1_wgrad_workspace_bytes", None, Bm, Co, Ci, L))
        if nbytes:
            ws = Out((nbytes // 4,))
        wp = None if (ws is None or fault == "null_workspace") else ws.ptr()
        if c.affine:
            rc = _lib.call("regnet_conv1x1_wgrad_bnrelu_f32", anchor, _p(inp, "dY"), _p(inp, "X"), out.ptr(off), B, Co, Ci, L,
                           _p(inp, "scale"), _p(inp, "shift"), c.relu, wp, tolerate=tolerate)
        else:
            rc = _lib.call("regnet_conv1x1_wgrad_f32", anchor, _p(inp, "dY"), _p(inp, "X"), out.ptr(off), B, Co, Ci, L, wp,
                           tolerate=tolerate)
    elif c.op == "smallci":
        out = Out((Bm, Co, L))
        if stats:
            sums = Out((2 * Co,), torch.float64)
            nbytes = int(_lib.call("regnet_conv1x1_smallci_stats_workspace_bytes", None, Bm, Ci, L))
            ws = Out((max(nbytes // 8, 1),), torch.float64)
            rc = _lib.call("regnet_conv1x1_fwd_smallci_stats_f32", anchor, _p(inp, "W"), _p(inp, "X"), out.ptr(off), B, Co, Ci, L,
                           ws.ptr(), sums.ptr(), tolerate=tolerate)
        else:
            rc = _lib.call("regnet_conv1x1_fwd_smallci_f32", anchor, _p(inp, "W"), _p(inp, "X"), out.ptr(off), B, Co, Ci, L,
                           tolerate=tolerate)
    elif c.op == "smallco":
        out = Out((Bm, Ci if c.direction else Co, L))
        rc = _lib.call("regnet_conv1x1_smallco_f32", anchor, c.direction, _p(inp, "W"), _p(inp, "bias") if c.bias else None,
                       _p(inp, "dY" if c.direction else "X"), out.ptr(off), B, Co, Ci, L, tolerate=tolerate)
    else:
        assert c.op == "wgrad_smallci", c.op
        parts = max(int(_lib.call("regnet_conv1x1_wgrad_smallci_partials", None, Bm, Co, L)), 1)
        out = Out((parts, Co, Ci))
        rc = _lib.call("regnet_conv1x1_wgrad_smallci_f32", anchor, _p(inp, "dY"), _p(inp, "X"), out.ptr(off), B, Co, Ci, L,
                       tolerate=tolerate)
    return Result(rc, out, sums, ws)


def check_guards(res, what):
    assert res.out.guards_intact(), "%s: a store outside the output" % what
    assert res.sums is None or res.sums.guards_intact(), "%s: a store outside the statistics" % what
    assert res.workspace is None or res.workspace.guards_intact(), "%s: a store outside the workspace" % what


def value(c, res):
    """The result of a call as the reference states it (float64 for the partial matrices of the small weight gradient)."""
    return res.out.body.double().sum(0) if c.op == "wgrad_smallci" else res.out.body


def same_bits(r1, r2, with_sums=True):
    """(with_sums=False: the fp64 atomics of the stream kernel add a float run's statistics in an order that varies)"""
    return torch.equal(r1.out.body.view(torch.int32), r2.out.body.view(torch.int32)) and (
        r1.sums is None or not with_sums or torch.equal(r1.sums.body.view(torch.int64), r2.sums.body.view(torch.int64)))


def describe_mismatch(got, want):
    bad = (got != want).nonzero()
    first = tuple(int(v) for v in bad[0])
    return "%d of %d elements differ, index ranges %s, first %s: got %r, want %r" % (
        bad.shape[0], got.numel(), [(int(bad[:, d].min()), int(bad[:, d].max())) for d in range(bad.shape[1])], first,
        float(got[first]), float(want[first]))


def check_exact(c, seed, what=None):
    what = what or c.id
    mode = "stats" if (c.stats and c.op == "fwd") else "exact"
    inp = make_inputs(c, mode, seed)
    want64, T = reference(c, inp)
    if c.op == "wgrad_smallci":     # every partial matrix is exact; the test adds them in float64
        n = cases.smallci_wgrad_slice_len(c.B, c.Co, c.L)
        assert float(inp["dY"].abs().max()) * float(inp["X"].abs().max()) * n < 2 ** 23
    else:
        assert float(T.max()) < 2 ** 23
    res = run(c, inp)
    assert res.rc == OK
    check_guards(res, what)
    got = value(c, res)
    want = want64 if c.op == "wgrad_smallci" else want64.float()
    assert torch.equal(got, want), "%s: %s" % (what, describe_mismatch(got, want))
    if c.stats:
        sums = res.sums.body.view(c.Co, 2)
        y = want64
        if c.op == "fwd":
            assert 64.0 * float((y * y).max()) <= 2 ** 24
        want_sums = torch.stack([y.sum(dim=(0, 2)), (y * y).sum(dim=(0, 2))], dim=1)
        assert float(want_sums.abs().max()) < 2 ** 53
        assert torch.equal(sums, want_sums), "%s: statistics: %s" % (what, describe_mismatch(sums, want_sums))
        plain = run(c, inp, stats=0)
        check_guards(plain, what)
        assert torch.equal(plain.out.body.view(torch.int32), res.out.body.view(torch.int32)), "%s: Y differs without statistics" % what
    again = run(c, inp)
    assert same_bits(res, again), "%s: two calls differ" % what
    if c.op in ("fwd", "dgrad") and not c.affine and not c.stats:
        tile = run(c, inp, entry="tile")
        check_guards(tile, what)
        assert same_bits(res, tile), "%s: stream and tile entry points differ" % what
    return res


def check_float(c, seed, what=None):
    what = what or c.id
    inp = make_inputs(c, "float", seed)
    want, T = reference(c, inp)
    tol = gref.gamma(roundings(c)) * T + (gref.U * T if c.affine else 0.0)
    res = run(c, inp)
    assert res.rc == OK
    check_guards(res, what)
    err = (value(c, res).double() - want).abs()
    assert bool(torch.isfinite(err).all()), "%s: non-finite output" % what
    ratio = float((err / tol.clamp_min(1e-300)).max())
    names = cases.instantiations(c)
    print("%s (%s): max error / tol = %.4f, max error %.3e" % (what, names[0], ratio, float(err.max())))
    _worst[names[0]] = max(_worst[names[0]], ratio)
    assert bool((err <= tol).all()), "%s: error / tol = %.3f" % (what, ratio)
    if c.stats and c.op == "fwd":
        y = res.out.body.double()
        sums = res.sums.body.view(c.Co, 2)
        for col, m in ((0, y.abs()), (1, y * y)):
            exact = (y if col == 0 else m).sum(dim=(0, 2))
            bound = (gref.gamma(8) + 1e-12) * m.sum(dim=(0, 2))
            r = float(((sums[:, col] - exact).abs() / bound.clamp_min(1e-300)).max())
            print("%s: statistics column %d: max error / tol = %.4f" % (what, col, r))
            _worst[names[0] + " sums"] = max(_worst[names[0] + " sums"], r)
            assert r <= 1.0, "%s: statistics column %d: error / tol = %.3f" % (what, col, r)
        plain = run(c, inp, stats=0)
        assert torch.equal(plain.out.body.view(torch.int32), res.out.body.view(torch.int32)), "%s: Y differs without statistics" % what
    again = run(c, inp)
    assert same_bits(res, again, with_sums=c.op != "fwd"), "%s: two calls differ" % what
    if len(names) == 2:
        tile = run(c, inp, entry="tile")
        check_guards(tile, what)
        _worst[names[1]] = max(_worst[names[1]], float(((tile.out.body.double() - want).abs() / tol.clamp_min(1e-300)).max()))
        assert same_bits(res, tile), "%s: stream and tile entry points differ" % what
    return res


# ------------------------------------------------------------------------------------------------------------------ tests
GEMM_IDS = [c.id for c in cases.GEMM_CASES]
SMALL_IDS = [c.id for c in cases.SMALL_CASES]


@pytest.mark.parametrize("case", cases.GEMM_CASES, ids=GEMM_IDS)
def test_exact_integers(case):
    check_exact(case, 1000 + GEMM_IDS.index(case.id))


@pytest.mark.parametrize("case", cases.GEMM_CASES, ids=GEMM_IDS)
def test_float_within_derived_bound(case):
    check_float(case, 2000 + GEMM_IDS.index(case.id))


@pytest.mark.parametrize("case", cases.SMALL_CASES, ids=SMALL_IDS)
def test_small_channel_exact_integers(case):
    check_exact(case, 3000 + SMALL_IDS.index(case.id))


@pytest.mark.parametrize("case", cases.SMALL_CASES, ids=SMALL_IDS)
def test_small_channel_float_within_derived_bound(case):
    check_float(case, 4000 + SMALL_IDS.index(case.id))


def stream_case(inst, K, M, B, L, what):
    op, affine, relu, stats = inst
    Co, Ci = (K, M) if op == "dgrad" else (M, K)
    return cases.Case(what, op, affine, relu, stats, B, Co, Ci, L, what, None, None, None, None, None)


def persistent_shape(which, grid):
    """-> (M, B, L) with total = tiles_m * tiles_n * B output tiles: "grid": exactly the grid (no workgroup draws a tile that
    exists); "grid+1": one workgroup computes a second tile, of another scene; "2.5grid": workgroups compute two or three tiles,
    34 or more per scene over three scenes.  Every point tile is ragged (L % 256 == 48 or 80)."""
    if which == "grid":
        assert grid % 2 == 0
        return cases.PERSISTENT_M, grid // 2, 80              # two channel tiles (128 + 32 rows) x one point tile per scene
    if which == "grid+1":
        return 48, grid + 1, 80                               # one partial channel tile x one point tile per scene
    B = 3
    tn = max(2, round(2.5 * grid / (2 * B)))
    while (2 * tn * B) % grid == 0 or grid % (2 * tn) == 0:
        tn += 1
    return cases.PERSISTENT_M, B, (tn - 1) * 256 + 48


def tiles_of(M, B, L):
    return ((M + 127) // 128) * ((L + 255) // 256) * B


@pytest.mark.parametrize("which", ["grid", "grid+1", "2.5grid"])
@pytest.mark.parametrize("K", cases.PERSISTENT_K)
@pytest.mark.parametrize("inst", cases.STREAM_INSTANTIATIONS, ids=["%s-a%d-r%d-s%d" % i for i in cases.STREAM_INSTANTIATIONS])
def test_persistent_workgroups_compute_further_tiles(inst, K, which):
    """Half the workgroup slots reserved (as the product does beside the region stage): the grid is the CU count, and the tiles
    beyond it are drawn from the ticket while the ring keeps running -- across a scene change for most of them."""
    from regnet_for_3d_grasping_amd import _lib
    cus = compute_units()
    before = _lib.call("regnet_conv1x1_stream_reserve_slots", None, cus)
    try:
        M, B, L = persistent_shape(which, cus)       # 2 x CUs slots, CUs of them reserved
        total = tiles_of(M, B, L)
        grid = min(total, cus)
        if which == "grid":
            assert total == grid
        else:
            assert total > grid
        if which == "2.5grid":
            assert total > 2 * grid and total % grid and grid % (tiles_of(M, 1, L)) and B >= 3
        what = "persistent %s %s K=%d" % ("-".join(str(v) for v in inst), which, K)
        _persistent.append((what, grid, total))
        c = stream_case(inst, K, M, B, L, what)
        check_exact(c, 5000 + K)
        if which == "2.5grid":
            check_float(c, 6000 + K)
    finally:
        _lib.call("regnet_conv1x1_stream_reserve_slots", None, before)


@pytest.mark.parametrize("inst", cases.STREAM_INSTANTIATIONS, ids=["%s-a%d-r%d-s%d" % i for i in cases.STREAM_INSTANTIATIONS])
def test_persistent_without_reservation(inst):
    """Two workgroups per CU, about 2.5 tiles each: M = 32, three scenes."""
    from regnet_for_3d_grasping_amd import _lib
    before = _lib.call("regnet_conv1x1_stream_reserve_slots", None, 0)
    try:
        _unreserved(inst)
    finally:
        _lib.call("regnet_conv1x1_stream_reserve_slots", None, before)


def _unreserved(inst):
    grid = 2 * compute_units()
    tn = round(2.5 * grid / 3)
    while (tn * 3) % grid == 0 or grid % tn == 0:
        tn += 1
    L = (tn - 1) * 256 + 48
    total = tiles_of(32, 3, L)
    assert total > 2 * grid
    what = "persistent %s unreserved K=32" % "-".join(str(v) for v in inst)
    _persistent.append((what, grid, total))
    c = stream_case(inst, 32, 32, 3, L, what)
    check_exact(c, 7000)
    check_float(c, 7001)


@pytest.mark.parametrize("rej", cases.REJECTS, ids=[r.id for r in cases.REJECTS])
def test_refusals(rej):
    """Refused on the host, before any launch: the status of the row, and every output still holds the sentinel.  (The buffers
    have the sizes of the refused shape.)"""
    c = cases.BY_ID[rej.base]._replace(**rej.override)
    inp = make_inputs(c, "exact", 8000)
    res = run(c, inp, fault=rej.fault, tolerate=rej.status)
    assert res.rc == rej.status, (rej.id, res.rc)
    assert res.out.untouched() and (res.sums is None or res.sums.untouched()) and (res.workspace is None or res.workspace.untouched())


@pytest.mark.parametrize("base", ["fwd-Co32-K32-L64", "aff-Co32-K32-L64-relu", "stat-Co32-K32-L64", "dgrad-Ci32-K32-L64",
                                  "smallci-Ci8-Co1-L4100", "smallco-Co4-Ci20-L8196-fwd", "wgrad-smallci-Ci8-Co1-L4100"])
def test_no_scene_is_success_and_touches_nothing(base):
    c = cases.BY_ID[base]._replace(B=0)
    inp = make_inputs(c, "exact", 9000)
    for entry in ("stream", "tile") if (c.op in ("fwd", "dgrad") and not c.affine and not c.stats) else ("stream",):
        res = run(c, inp, entry=entry)
        assert res.rc == OK
        assert res.out.untouched() and (res.sums is None or res.sums.untouched()) and (res.workspace is None or res.workspace.untouched())


def test_weight_gradient_refuses_no_scene():
    """B == 0 has no weight gradient: include/regnet_hip.h's wgrad sums over at least one scene (REGNET_ERR_SHAPE)."""
    c = cases.BY_ID["wgrad-n1"]._replace(B=0)
    res = run(c, make_inputs(c, "exact", 9001), tolerate=cases.ERR_SHAPE)
    assert res.rc == cases.ERR_SHAPE and res.out.untouched()
