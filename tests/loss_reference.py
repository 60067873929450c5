"""The contract of the loss and label kernels (csrc/losses.hip: regnet_stage2_loss_rows_f32, regnet_ce_rows_f32,
regnet_refine_loss_rows_f32, regnet_label_match_f32) restated in numpy from include/regnet_hip.h and the kernel comments.

Two passes over the same float32 inputs:

  decisions   in float32, in the kernel's operation order, every operation rounded on its own (numpy rounds each float32
              operation; losses.hip is built with -ffp-contract=off): the arg-max class ``pick`` (first maximum), the label's
              anchor ``g8`` (first minimum of 1 - cos), terms[8]; the three refine flags and terms[16..19]; the matched grasp
              (first minimum of the float32 expansion compared as float64), ``has`` (distance <= max_sq, inclusive), ``flip``,
              ``missing``, ``wide_row`` and the branch of each of the four theta wrap steps.  These are compared exactly.
  values      in float64 from the float32 inputs, with the decisions of the first pass: terms, next_grasp, final_grasp, a_gt,
              dreg, the cross entropy and dcls, theta.  Every value is a ``V``: the float64 value, its MAGNITUDE (the same
              expression with |.| taken at every addition and subtraction) and ``k``, the number of float32 roundings on its
              longest path, so that the kernel's float32 result lies within ``k * 2^-24 * magnitude`` (first order in 2^-24).

How k is counted (``V`` does it while it evaluates, the tables K_* below state the result per output and
tests/test_loss_reference_cpu.py asserts that both agree): an input or a float32 constant has k = 0; a sum or difference has
max(k_a, k_b) + 1 and magnitude mag_a + mag_b; a product or quotient inherits the RELATIVE errors of both operands,
k_a + k_b + 1, magnitude mag_a mag_b (quotient: mag_a mag_b / b^2, which is mag_a / |b| for the denominators here, all square
roots of sums of squares); a square root halves the relative error, ceil(k_a / 2) + 1; a product with a power of two, a
negation and 0 + x are exact.  smooth-L1 is continuous with a continuous derivative, so the side of |e| = 1 taken by a float32
e within its bound of 1 does not matter to either: 0.5 e^2 has 2 k_e + 1, |e| - 0.5 has k_e + 1 (the larger is used) and
SL1'(e) = clip(e, -1, 1) has k_e.  expf, logf and atan2f are not counted here: the tests measure torch's float32 log_softmax /
softmax / atan2 against float64 on the same inputs and allow the kernel twice that plus one ulp of the result.

The second half builds the edge-case inputs for a comparison with the kernels; tests/test_loss_reference_cpu.py asserts on the
CPU that each of them holds its case (a float32 value exactly on the threshold and on both sides of it, a tie set, an empty
class, ...).
"""
import numpy as np

f32, f64 = np.float32, np.float64
U = 2.0 ** -24
PI32, TWO_PI32 = f32(3.14159265358979323846), f32(6.28318530717958647692)
EPS32 = f32(1e-12)
S = f32(0.5771484375)                                   # the fp16 template entry (gripper_region_network._enumerate_templates)
TEMPLATES = np.array([[S, S, S, 0], [S, S, -S, 0], [S, -S, -S, 0], [S, -S, S, 0]], dtype=f32)
NEAR_T, ALIGNED_T, ANGLE_T = f32(0.025), f32(0.5), f32(1.047)
S2_TERMS, RF_TERMS = 12, 20


def nudge(x, steps):
    """x (float32 array or scalar) moved by ``steps`` (integer array or scalar) float32 neighbours."""
    x = np.asarray(x, dtype=f32)
    bits = x.view(np.int32).astype(np.int64)
    key = np.where(bits < 0, -(bits & 0x7fffffff), bits) + np.asarray(steps, dtype=np.int64)     # monotone integer key
    back = np.where(key < 0, (-key) | 0x80000000, key).astype(np.uint32)
    return back.view(f32)


def ulp32(x):
    """The spacing of float32 at |x| (float64)."""
    x = np.abs(np.asarray(x, dtype=f64)).astype(f32)
    return (nudge(x, 1).astype(f64) - x.astype(f64))


# ---- float64 values with magnitude and rounding count ------------------------------------------------------------------------
class V:
    """value, magnitude, k -- see the module docstring."""
    __slots__ = ("val", "mag", "k")

    def __init__(self, val, mag=None, k=0):
        self.val = np.asarray(val, dtype=f64)
        self.mag = np.abs(self.val) if mag is None else np.asarray(mag, dtype=f64)
        self.k = int(k)

    @staticmethod
    def of(x):
        return x if isinstance(x, V) else V(x)

    def __add__(self, o):
        o = V.of(o)
        return V(self.val + o.val, self.mag + o.mag, max(self.k, o.k) + 1)

    def __sub__(self, o):
        o = V.of(o)
        return V(self.val - o.val, self.mag + o.mag, max(self.k, o.k) + 1)

    def __rsub__(self, o):
        return V.of(o) - self

    def __mul__(self, o):
        o = V.of(o)
        return V(self.val * o.val, self.mag * o.mag, self.k + o.k + 1)

    def __truediv__(self, o):
        o = V.of(o)
        return V(self.val / o.val, self.mag * o.mag / (o.val * o.val), self.k + o.k + 1)

    def sqrt(self):
        r = np.sqrt(self.val)
        return V(r, self.mag / r, (self.k + 1) // 2 + 1)

    def exact(self, factor):
        return V(self.val * factor, self.mag * abs(factor), self.k)

    def abs(self):
        return V(np.abs(self.val), self.mag, self.k)

    def masked(self, keep):
        """zero (exactly) where ``keep`` is False."""
        return V(np.where(keep, self.val, 0.0), np.where(keep, self.mag, 0.0), self.k)

    @property
    def bound(self):
        return self.k * U * self.mag


def where(cond, a, b):
    a, b = V.of(a), V.of(b)
    return V(np.where(cond, a.val, b.val), np.where(cond, a.mag, b.mag), max(a.k, b.k))


class Table:
    """columns of V (each (m,)) -> val / mag / bound (m, cols) and k per column."""

    def __init__(self, cols):
        cols = [V.of(c) for c in cols]
        self.val = np.stack([c.val for c in cols], axis=-1)
        self.mag = np.stack([c.mag for c in cols], axis=-1)
        self.k = [c.k for c in cols]
        self.bound = self.mag * (np.asarray(self.k, dtype=f64) * U)

    def column_sums(self, n_terms=None):
        """the float32 sum of the rows in any order: (rows - 1) further roundings on the longest path."""
        m = self.val.shape[0] if n_terms is None else n_terms
        return [V(self.val[:, j].sum(), self.mag[:, j].sum(), self.k[j] + max(m - 1, 0)) for j in range(self.val.shape[1])]


def sl1_v(e):
    quad = (e * e).exact(0.5)
    lin = e.abs() - 0.5
    return where(np.abs(e.val) < 1.0, quad, V(lin.val, lin.mag, quad.k))


def sl1_grad_v(e):
    return V(np.clip(e.val, -1.0, 1.0), e.mag, e.k)


def sum3(a, b, c):
    return (a + b) + c


def one_minus_cos_v(a, b):
    """a, b: lists of three V."""
    dot = sum3(a[0] * b[0], a[1] * b[1], a[2] * b[2])
    na = sum3(a[0] * a[0], a[1] * a[1], a[2] * a[2]) + f64(EPS32)
    nb = sum3(b[0] * b[0], b[1] * b[1], b[2] * b[2]) + f64(EPS32)
    return 1.0 - dot / (na * nb).sqrt()


# ---- float32 pieces (decisions) ----------------------------------------------------------------------------------------------
def sl1_32(x):
    x = np.asarray(x, dtype=f32)
    a = np.abs(x)
    return np.where(a < f32(1), f32(0.5) * x * x, a - f32(0.5)).astype(f32)


def sl1_grad_32(x):
    x = np.asarray(x, dtype=f32)
    return np.where(np.abs(x) < f32(1), x, np.where(x > 0, f32(1), f32(-1))).astype(f32)


def one_minus_cos_32(a, b):
    """a, b (..., 3) float32 -> 1 - dot / sqrt((|a|^2 + 1e-12) (|b|^2 + 1e-12)), the kernel's order."""
    a, b = np.asarray(a, dtype=f32), np.asarray(b, dtype=f32)
    dot = (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]
    na = ((a[..., 0] * a[..., 0] + a[..., 1] * a[..., 1]) + a[..., 2] * a[..., 2]) + EPS32
    nb = ((b[..., 0] * b[..., 0] + b[..., 1] * b[..., 1]) + b[..., 2] * b[..., 2]) + EPS32
    return f32(1) - dot / np.sqrt(na * nb)


def anchor_similarity_32(tmpl, axis):
    """tmpl (A, 4), axis (m, 3) -> (m, A) float32 1 - cos of every template axis with the label's axis."""
    tmpl = np.asarray(tmpl, dtype=f32)
    return np.stack([one_minus_cos_32(tmpl[a, :3][None, :], axis) for a in range(tmpl.shape[0])], axis=1)


def axis_norm_32(g3, tp3):
    ax = g3 + tp3
    return np.sqrt(((ax[..., 0] * ax[..., 0] + ax[..., 1] * ax[..., 1]) + ax[..., 2] * ax[..., 2]) + EPS32), ax


def stage2_errors_32(g, c, tp, gt, radius):
    """The ten float32 errors e of the label's anchor: g (m,10) its regression, c (m,3), tp (m,4), gt (m,10)."""
    g, c, tp, gt, radius = (np.asarray(x, dtype=f32) for x in (g, c, tp, gt, radius))
    e = np.empty(g.shape, dtype=f32)
    e[..., 0:3] = g[..., 0:3] - (gt[..., 0:3] - c[..., 0:3]) / radius
    n, _ = axis_norm_32(g[..., 3:6], tp[..., 0:3])
    e[..., 3:6] = g[..., 3:6] * n[..., None] - (gt[..., 3:6] - tp[..., 0:3])
    e[..., 6] = g[..., 6] - (gt[..., 6] - tp[..., 3]) / PI32
    e[..., 7:10] = g[..., 7:10] - gt[..., 7:10]
    return e


# rounding counts, per output column, as ``V`` finds them (asserted equal in tests/test_loss_reference_cpu.py)
# next_grasp: r * radius + c: 2; axis / norm: (r + tp) 1, squares 3, two sums 5, + eps 6, sqrt 4, quotient 1 + 4 + 1 = 6;
#             pi (r + tp): 2; scores are copies
K_NEXT_GRASP = [2, 2, 2, 6, 6, 6, 2, 0, 0, 0]
# terms 0: e = g - (gt - c) / radius: 3, SL1 7, two sums 9.   1: n 4, g n 5, e 6, SL1 13, sums 15.   2: e 3, SL1 7.
#       3: e 1, SL1 3, sums 5.   4: (o - gt) 3, SL1 7, sums 9.   5: 1 - cos of the decoded axis (k 6): dot 7 + 2 = 9,
#       |o|^2 13 + 3 = 16, |gt|^2 4, product 21, sqrt 12, quotient 22, 1 - . 23.   6: (o6 - gt6) 3, SL1 7.   7: as 3.   8..11: exact
K_S2_TERMS = [9, 15, 7, 5, 9, 23, 7, 5, 0, 0, 0, 0]
# dreg 0..2: w0 SL1'(e): 3 + 1.   3..5: SL1'(e) n: 6 + 4 + 1 = 11; gdot: products 7, sums 9; axis / n: 1 + 4 + 1 = 6;
#      gdot (axis / n): 16; sum 17; w1 .: 18.   6: 3 + 1.   7..9: 1 + 1
K_S2_DREG = [4, 4, 4, 18, 18, 18, 4, 2, 2, 2]
# final: g + r radius: 2; g + r: 1
K_FINAL = [2, 2, 2, 1, 1, 1, 1, 1, 1, 1]
# refine terms 0: tgt (gt - g) / radius 2, e 3, SL1 7, the sum starts at 0: two roundings, 9.   1: tgt 1, e 2, SL1 5, 7.
#       2: SL1 5 (0 + x is exact).   3: 7.   4..7 (stage-2 grasp): (p - gt) 1, SL1 3, sums 5 | 1 - cos of inputs: dot 3, norms 4,
#       product 9, sqrt 6, quotient 10, 11 | SL1 3 | 5.   8..15 (final grasp, centre k 2, others k 1): 3, 7, 9 | dot 4, |o|^2 6,
#       |gt|^2 4, product 11, sqrt 7, quotient 12, 13 | (o6 - gt6) 2, SL1 5 | 2, 5, 7.   16..19: exact
K_RF_TERMS = [9, 7, 5, 7, 5, 11, 3, 5, 9, 13, 5, 7, 9, 13, 5, 7, 0, 0, 0, 0]
K_RF_DREG = [3, 3, 3, 2, 2, 2, 2, 2, 2, 2]


def stage2_rows(cls, reg, centre, tmpl, label, radius, weights, rows=None):
    """regnet_stage2_loss_rows_f32.  cls (n,A), reg (n,A,10), centre (n, >= 3), tmpl (A,4), label (n, >= 10) float32,
    weights (4), rows (m) or None.  -> dict: pick, g8 (m) int32, a_gt (m,7) float32 (copies), equal (m) = terms[8],
    next_grasp / terms / dreg as ``Table`` (dreg: the ten entries of anchor g8; every other anchor's are exact zeros),
    e32 (m,10) the float32 errors and dreg32_linear (m,10): +-w where |e32| >= 1, nan elsewhere."""
    cls, reg, centre, tmpl, label = (np.asarray(x, dtype=f32) for x in (cls, reg, centre, tmpl, label))
    n, A = cls.shape
    rows = np.arange(n) if rows is None else np.asarray(rows, dtype=np.int64)
    m = len(rows)
    radius = f32(radius)
    w = np.asarray(weights, dtype=f32)
    cl, c, gt, rg = cls[rows], centre[rows, :3], label[rows, :10], reg[rows]
    pick = np.argmax(cl, axis=1).astype(np.int32)                      # first maximum
    g8 = np.argmin(anchor_similarity_32(tmpl, gt[:, 3:6]), axis=1).astype(np.int32)    # first minimum
    ar = np.arange(m)
    a_gt = np.concatenate([c, tmpl[g8]], axis=1)
    col = lambda x: [V(x[:, j]) for j in range(x.shape[1])]
    cv, gtv = col(c), col(gt)
    # ---- arg-max decode and its monitoring terms
    r, tp = col(rg[ar, pick]), col(tmpl[pick])
    o = [r[k] * f64(radius) + cv[k] for k in range(3)]
    ax = [r[3 + k] + tp[k] for k in range(3)]
    norm = (sum3(ax[0] * ax[0], ax[1] * ax[1], ax[2] * ax[2]) + f64(EPS32)).sqrt()
    o += [ax[k] / norm for k in range(3)]
    o.append(V(f64(PI32)) * (r[6] + tp[3]))
    o += r[7:10]
    t = [None] * S2_TERMS
    t[4] = sum3(*[sl1_v(o[k] - gtv[k]) for k in range(3)])
    t[5] = one_minus_cos_v(o[3:6], gtv[3:6])
    t[6] = sl1_v(o[6] - gtv[6])
    t[7] = sum3(*[sl1_v(o[k] - gtv[k]) for k in range(7, 10)])
    equal = (g8 == pick)
    t[8] = V(equal.astype(f64))
    t[9] = t[10] = t[11] = V(np.zeros(m))
    # ---- the label's anchor
    g, tp = col(rg[ar, g8]), col(tmpl[g8])
    d = [None] * 10
    e0 = [g[k] - (gtv[k] - cv[k]) / f64(radius) for k in range(3)]
    t[0] = sum3(*[sl1_v(e) for e in e0])
    for k in range(3):
        d[k] = V(f64(w[0])) * sl1_grad_v(e0[k])
    ax = [g[3 + k] + tp[k] for k in range(3)]
    nn = (sum3(ax[0] * ax[0], ax[1] * ax[1], ax[2] * ax[2]) + f64(EPS32)).sqrt()
    e1 = [g[3 + k] * nn - (gtv[3 + k] - tp[k]) for k in range(3)]
    t[1] = sum3(*[sl1_v(e) for e in e1])
    ge = [sl1_grad_v(e) for e in e1]
    gdot = sum3(*[ge[k] * g[3 + k] for k in range(3)])
    for k in range(3):
        d[3 + k] = V(f64(w[1])) * (ge[k] * nn + gdot * (ax[k] / nn))
    e6 = g[6] - (gtv[6] - tp[3]) / f64(PI32)
    t[2] = sl1_v(e6)
    d[6] = V(f64(w[2])) * sl1_grad_v(e6)
    e3 = [g[k] - gtv[k] for k in range(7, 10)]
    t[3] = sum3(*[sl1_v(e) for e in e3])
    for k in range(3):
        d[7 + k] = V(f64(w[3])) * sl1_grad_v(e3[k])
    e32 = stage2_errors_32(rg[ar, g8], c, tmpl[g8], gt, radius)
    wcol = w[[0, 0, 0, 1, 1, 1, 2, 3, 3, 3]]
    linear = np.where(np.abs(e32) >= 1, np.where(e32 > 0, wcol, -wcol), f32(np.nan)).astype(f32)
    linear[:, 3:6] = np.nan          # (the axis gradient is a combination of SL1' values: never +-w by itself)
    return dict(rows=rows, pick=pick, g8=g8, a_gt=a_gt, equal=equal, next_grasp=Table(o), terms=Table(t), dreg=Table(d),
                e32=e32, dreg32_linear=linear)


def ce_rows(cls, target, idx, rows, scale):
    """regnet_ce_rows_f32 in float64: -> loss (nb), dcls (n, A) (zero on the rows not drawn), drawn (n) bool."""
    cls = np.asarray(cls, dtype=f32)
    idx = np.asarray(idx, dtype=np.int64)
    r = idx if rows is None else np.asarray(rows, dtype=np.int64)[idx]
    x = cls[r].astype(f64)
    tg = np.asarray(target)[idx].astype(np.int64)
    mx = x.max(axis=1, keepdims=True)
    lse = np.log(np.exp(x - mx).sum(axis=1)) + mx[:, 0]
    loss = lse - x[np.arange(len(idx)), tg]
    soft = np.exp(x - lse[:, None])
    soft[np.arange(len(idx)), tg] -= 1.0
    dcls = np.zeros(cls.shape, dtype=f64)
    dcls[r] = soft * f64(f32(scale))
    drawn = np.zeros(cls.shape[0], dtype=bool)
    drawn[r] = True
    return loss, dcls, drawn


def refine_flags_32(grasp, cls, reg, label, radius, score_thre):
    """The float32 decisions of refine_loss_rows_kernel: -> one, kept, pos (m) bool and the three compared float32 values."""
    grasp, cls, reg, label = (np.asarray(x, dtype=f32) for x in (grasp, cls, reg, label))
    o7 = grasp[:, 7] + reg[:, 7]
    one = cls[:, 1] > cls[:, 0]
    kept = one & (o7 > f32(score_thre))
    off = grasp[:, :3] - label[:, :3]
    dist = np.sqrt((off[:, 0] * off[:, 0] + off[:, 1] * off[:, 1]) + off[:, 2] * off[:, 2])
    sim = one_minus_cos_32(grasp[:, 3:6], label[:, 3:6])
    dth = np.abs(grasp[:, 6] - label[:, 6])
    pos = (dist < NEAR_T) & (sim < ALIGNED_T) & (dth < ANGLE_T)
    return one, kept, pos, dist, sim, dth, o7


def refine_rows(grasp, cls, reg, label, radius, score_thre):
    """regnet_refine_loss_rows_f32.  grasp (m, >= 10), cls (m,2), reg (m,10), label (m, >= 10) -> dict: flags (3,m) uint8,
    final / terms / dreg as ``Table`` (dreg unscaled: SL1'(e) of a label-positive row, exact zeros otherwise)."""
    grasp, cls, reg, label = (np.asarray(x, dtype=f32) for x in (grasp, cls, reg, label))
    m = reg.shape[0]
    one, kept, pos, _, _, _, _ = refine_flags_32(grasp, cls, reg, label, radius, score_thre)
    col = lambda x: [V(x[:, j]) for j in range(10)]
    g, r, gt = col(grasp), col(reg), col(label)
    rad = f64(f32(radius))
    o = [g[k] + r[k] * rad for k in range(3)] + [g[k] + r[k] for k in range(3, 10)]
    e = [r[k] - ((gt[k] - g[k]) / rad if k < 3 else gt[k] - g[k]) for k in range(10)]
    s = [sl1_v(x).masked(pos) for x in e]
    t = [None] * RF_TERMS
    plus = lambda a, b, c: V(a.val + b.val + c.val, a.mag + b.mag + c.mag, max(a.k, b.k, c.k) + 2)   # 0 + a is exact
    t[0], t[1], t[2], t[3] = plus(*s[0:3]), plus(*s[3:6]), s[6], plus(*s[7:10])
    d = [sl1_grad_v(x).masked(pos) for x in e]
    for q, (p, use) in enumerate(((g, one), (o, one), (o, kept))):
        tq = [sum3(*[sl1_v(p[k] - gt[k]) for k in range(3)]), one_minus_cos_v(p[3:6], gt[3:6]), sl1_v(p[6] - gt[6]),
              sum3(*[sl1_v(p[k] - gt[k]) for k in range(7, 10)])]
        for j in range(4):
            t[4 + 4 * q + j] = tq[j].masked(use)
    for j, flag in enumerate((pos & one, ~pos & ~one, ~pos & one, pos & ~one)):
        t[16 + j] = V(flag.astype(f64))
    flags = np.stack([one, kept, pos]).astype(np.uint8)
    return dict(flags=flags, one=one, kept=kept, pos=pos, final=Table(o), terms=Table(t), dreg=Table(d))


# ---- label matching ------------------------------------------------------------------------------------------------------------
def contact_points_32(packed, depth):
    """packed (..., 19) -> (..., 3): (c + approach * depth) - approach * depth, each operation rounded."""
    packed = np.asarray(packed, dtype=f32)
    t = packed[..., [0, 4, 8]] * f32(depth)
    return (packed[..., [3, 7, 11]] + t) - t


def match_distance_32(a, cp):
    """a (3,), cp (G, 3) float32 -> the reference's expansion -2 a.cp + |cp|^2 + |a|^2 in float32."""
    a, cp = np.asarray(a, dtype=f32), np.asarray(cp, dtype=f32)
    aa = (a[0] * a[0] + a[1] * a[1]) + a[2] * a[2]
    dot = (a[0] * cp[:, 0] + a[1] * cp[:, 1]) + a[2] * cp[:, 2]
    bb = (cp[:, 0] * cp[:, 0] + cp[:, 1] * cp[:, 1]) + cp[:, 2] * cp[:, 2]
    d = f32(-2) * dot
    d = d + bb
    return d + aa


WRAP_LINES = (float(TWO_PI32), -float(TWO_PI32), float(PI32), -float(PI32))


def wrap_theta(a32, a64, flip):
    """atan2 as float32 (decisions) and float64 (value) -> theta float32 pass, theta float64, its magnitude, the number of
    additions made, and whether a compared float64 value lies within 4 float32 ulps of its wrap line."""
    a32 = np.asarray(a32, dtype=f32)
    th32 = np.where(flip, PI32 - a32, a32).astype(f32)
    th = np.where(flip, f64(PI32) - a64, a64)
    mag = np.where(flip, f64(PI32) + np.abs(a64), np.abs(a64))
    adds = flip.astype(np.int64)
    close = np.zeros(a32.shape, dtype=bool)
    steps = ((lambda x: x >= TWO_PI32, -1), (lambda x: x <= -TWO_PI32, 1), (lambda x: x > PI32, -1), (lambda x: x <= -PI32, 1))
    for (test, sign), line in zip(steps, WRAP_LINES):
        close |= np.abs(th - line) <= 4 * ulp32(line)
        take = test(th32)
        th32 = np.where(take, th32 + f32(sign) * TWO_PI32, th32).astype(f32)
        th = np.where(take, th + sign * f64(TWO_PI32), th)
        mag = np.where(take, mag + f64(TWO_PI32), mag)
        adds = adds + take
    return th32, th, mag, adds, close


def label_match(packed, gcount, centre, depth, max_sq):
    """regnet_label_match_f32.  packed (B, Gmax, 19) float32, gcount (B), centre (B, Nc, >= 3) float32, max_sq float64 ->
    dict: index (B,Nc) (first minimum; -1 without a grasp), best (B,Nc) float64, has, flip, missing (B,Nc) bool, wide_row
    (B,Nc) int32, out (B,Nc,10) float32 whose columns other than 6 are what the kernel must write bit for bit, theta
    (float64), theta_mag, theta_adds, atan_x / atan_y (the float32 arguments of atan2) and near_wrap."""
    packed, centre = np.asarray(packed, dtype=f32), np.asarray(centre, dtype=f32)
    B, Nc = centre.shape[:2]
    index = np.full((B, Nc), -1, dtype=np.int64)
    best = np.full((B, Nc), np.inf, dtype=f64)
    for b in range(B):
        G = int(gcount[b])
        if G == 0:
            continue
        cp = contact_points_32(packed[b, :G], depth)
        for c in range(Nc):
            d = match_distance_32(centre[b, c, :3], cp).astype(f64)
            index[b, c] = int(np.argmin(d))                            # first minimum
            best[b, c] = d[index[b, c]]
    has = (index >= 0) & (best <= f64(max_sq))
    rec = np.full((B, Nc, 19), -1.0, dtype=f32)
    for b, c in zip(*np.nonzero(has)):
        rec[b, c] = packed[b, index[b, c]]
    fx, fy, fz, fc = rec[..., [0, 4, 8]], rec[..., [1, 5, 9]], rec[..., [2, 6, 10]], rec[..., [3, 7, 11]]
    missing = (fx == f32(-1)).all(axis=-1)
    flip = fy[..., 0] < 0
    with np.errstate(all="ignore"):
        a32 = np.arctan2(fx[..., 2], fz[..., 2])
        a64 = np.arctan2(fx[..., 2].astype(f64), fz[..., 2].astype(f64))
    th32, th, mag, adds, close = wrap_theta(a32, a64, flip)
    th32 = np.where(missing, f32(-1), th32).astype(f32)
    th = np.where(missing, -1.0, th)
    out = np.empty((B, Nc, 10), dtype=f32)
    out[..., 0:3] = fc
    out[..., 3:6] = np.where(flip[..., None], -fy, fy)
    out[..., 6] = th32
    out[..., 7:10] = rec[..., 16:19]
    return dict(index=index, best=best, has=has, flip=flip, missing=missing, wide_row=(rec[..., 17] != f32(-1)).astype(np.int32),
                out=out, theta=th, theta_mag=mag, theta_adds=adds, atan_y=fx[..., 2], atan_x=fz[..., 2],
                near_wrap=close & ~missing)


# ---- the host side of region_losses (class balancing on numpy's global stream) ---------------------------------------------------
def _weights(m):
    return np.array([10.0 / (3 * m), 5.0 / (3 * m), 1.0 / m, 1.0 / (3 * m)]).astype(f32)


def _scaled(v, s):
    return v * V(f64(f32(s)))


def stage2_loss(cls, reg, centre, tmpl, ground, radius):
    """region_losses.stage2_loss with numpy's global generator where the host draws.  ground (n, >= 10) label rows; a row is
    labelled when its last column is not -1.  -> dict: rows, row results (``rows_out``), idx (the drawn compact positions),
    values (12 V: the scaled column sums; [9] the count of g8 != pick, [10] left to the caller's cross entropy), ce_rows / dcls
    from ``ce_rows`` with scale 1 / nb, regression loss = 10 v0 + 5 v1 + v2 + v3 as V, dreg (n, A, 10) value and bound."""
    cls, reg, ground = np.asarray(cls, dtype=f32), np.asarray(reg, dtype=f32), np.asarray(ground, dtype=f32)
    n, A = cls.shape
    rows = np.nonzero(ground[:, -1] != -1)[0]
    m = len(rows)
    out = stage2_rows(cls, reg, centre, tmpl, ground, radius, _weights(m), rows)
    members = [np.nonzero(out["g8"] == a)[0] for a in range(A)]
    per_class = max(int(min(len(mem) for mem in members)), 1)
    idx = np.concatenate([mem[np.random.choice(len(mem), per_class, replace=False)] for mem in members if len(mem)])
    nb = len(idx)
    loss_rows, dcls, drawn = ce_rows(cls, out["g8"], idx, rows, 1.0 / nb)
    sums = out["terms"].column_sums()
    scale = [1.0 / (3 * m), 1.0 / (3 * m), 1.0 / m, 1.0 / (3 * m), 1.0 / (3 * m), 1.0 / m, 1.0 / m, 1.0 / (3 * m)]
    values = [_scaled(sums[j], scale[j]) for j in range(8)]
    count = float(out["equal"].sum())
    values += [V(count), V(m - count), None, V(0.0)]
    # the dot product with (10, 5, 1, 1, ..., 1 at the cross entropy): twelve products and eleven sums at most
    reg_loss = V(10 * values[0].val + 5 * values[1].val + values[2].val + values[3].val,
                 10 * values[0].mag + 5 * values[1].mag + values[2].mag + values[3].mag,
                 max(v.k for v in values[:4]) + 1 + 11)
    dreg = np.zeros((n, A, 10), dtype=f64)
    dreg_bound = np.zeros((n, A, 10), dtype=f64)
    dreg[rows, out["g8"]] = out["dreg"].val
    dreg_bound[rows, out["g8"]] = out["dreg"].bound
    return dict(rows=rows, m=m, rows_out=out, members=members, per_class=per_class, idx=idx, nb=nb, values=values,
                ce_rows=loss_rows, ce=loss_rows.mean(), dcls=dcls, drawn=drawn, reg_loss=reg_loss, dreg=dreg,
                dreg_bound=dreg_bound)


def refine_loss(grasp, cls, reg, label, radius, score_thre):
    """region_losses.refine_loss: -> dict with the branch taken (num, P, nc, ns), values (16 V or nan), counts, idx, ce_rows,
    dcls, regression loss as V, dreg value / bound (m, 10), final, class_select, score_select."""
    out = refine_rows(grasp, cls, reg, label, radius, score_thre)
    m = out["flags"].shape[1]
    class_np, score_np = np.nonzero(out["one"])[0], np.nonzero(out["kept"])[0]
    pos_np, neg_np = np.nonzero(out["pos"])[0], np.nonzero(~out["pos"])[0]
    num = min(len(neg_np), len(pos_np))
    P, nc, ns = len(pos_np), len(class_np), len(score_np)
    sums = out["terms"].column_sums()
    nan = float("nan")
    reg_scale = [1.0 / (3 * P), 1.0 / (3 * P), 1.0 / P, 1.0 / (3 * P)] if num > 0 else [0.0] * 4
    if nc > 0:
        mon = [1.0 / (3 * nc), 1.0 / nc, 1.0 / nc, 1.0 / (3 * nc)] * 2 + \
              ([1.0 / (3 * ns), 1.0 / ns, 1.0 / ns, 1.0 / (3 * ns)] if ns > 0 else [nan] * 4)
    else:
        mon = [0.0] * 12
    values = [_scaled(sums[j], s) for j, s in enumerate(reg_scale + mon)]
    res = dict(rows_out=out, num=num, P=P, nc=nc, ns=ns, values=values, counts=[float(s.val) for s in sums[16:20]],
               class_select=class_np, score_select=score_np, idx=None, ce_rows=None, ce=0.0,
               dcls=np.zeros((m, 2)), drawn=np.zeros(m, dtype=bool), dreg=np.zeros((m, 10)), dreg_bound=np.zeros((m, 10)),
               reg_loss=V(0.0))
    if num > 0:
        idx0 = neg_np[np.random.choice(len(neg_np), num, replace=False)]
        idx1 = pos_np[np.random.choice(len(pos_np), num, replace=False)]
        idx = np.concatenate((idx0, idx1))
        loss_rows, dcls, drawn = ce_rows(cls, out["pos"].astype(np.int32), idx, None, 1.0 / len(idx))
        colscale = np.array(reg_scale[:1] * 3 + reg_scale[1:2] * 3 + reg_scale[2:3] + reg_scale[3:4] * 3).astype(f32).astype(f64)
        res.update(idx=idx, ce_rows=loss_rows, ce=loss_rows.mean(), dcls=dcls, drawn=drawn,
                   dreg=out["dreg"].val * colscale, dreg_bound=(out["dreg"].bound + U * out["dreg"].mag) * colscale,
                   reg_loss=V(sum(v.val for v in values[:4]), sum(v.mag for v in values[:4]), max(v.k for v in values[:4]) + 3))
    return res


# ================================================================================================================================
# input builders
# ================================================================================================================================
PREV1, NEXT1 = nudge(f32(1), -1), nudge(f32(1), 1)
SL1_TARGETS = np.array([0, 0.5, PREV1, 1, NEXT1, 3, -0.0, -0.5, -PREV1, -1, -NEXT1, -3], dtype=f32)
SL1_BOUNDARY = np.array([abs(float(t)) in (float(PREV1), 1.0, float(NEXT1)) for t in SL1_TARGETS])
SL1_GROUPS = {0: (0, 1, 2), 1: (3, 4, 5), 2: (6,), 3: (7, 8, 9)}


def unit_rows(rng, n):
    v = rng.normal(0, 1, (n, 3))
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(f32)


def random_labels(rng, n, centres):
    """label rows as the dataset makes them: a centre near the point, a unit axis with x >= 0, an angle, three scores."""
    axis = unit_rows(rng, n)
    axis = np.where(axis[:, :1] < 0, -axis, axis)
    return np.concatenate([centres[:, :3] + rng.normal(0, 0.01, (n, 3)).astype(f32), axis,
                           rng.normal(0, 0.8, (n, 1)).astype(f32), rng.uniform(0, 1, (n, 3)).astype(f32)], axis=1).astype(f32)


def templates(A, seed=0):
    """(A, 4) float32: the network's four first, then fp16-rounded random unit axes with a template angle."""
    if A <= 4:
        return TEMPLATES[:A].copy()
    rng = np.random.default_rng(1000 + seed + A)
    extra = np.concatenate([unit_rows(rng, A - 4), rng.uniform(-0.5, 0.5, (A - 4, 1)).astype(f32)], axis=1)
    return np.concatenate([TEMPLATES, extra.astype(np.float16).astype(f32)], axis=0)


def stage2_case(n, A, seed, labelled=0.8, centre_ld=3, label_ld=10, spread=0.3):
    """Random stage-2 inputs: -> cls (n,A), reg (n,A,10), centre (n,centre_ld), tmpl (A,4), label (n,label_ld); a fraction
    ``labelled`` of the rows carries a label, the others the dataset's filler (-1, axis +1).  ``spread`` 1.5 puts a third of
    the errors beyond the quadratic zone."""
    rng = np.random.default_rng(seed)
    centre = np.full((n, centre_ld), 9.0, dtype=f32)
    centre[:, :3] = rng.normal(0, 0.2, (n, 3))
    label = np.full((n, label_ld), -1.0, dtype=f32)
    label[:, 3:6] = 1.0
    has = rng.uniform(0, 1, n) < labelled
    if n and not has.any():
        has[0] = True
    label[has, :10] = random_labels(rng, int(has.sum()), centre[has])
    if label_ld > 10:
        label[:, 10:] = 5.0
        label[has, -1] = 0.25
        label[~has, -1] = -1.0
    return (rng.normal(0, 1, (n, A)).astype(f32), (rng.normal(0, spread, (n, A, 10))).astype(f32), centre, templates(A, seed),
            label)


def _solve_axis(v, tp):
    """float64: g with g |g + tp| = v (bisection on n = |g + tp|)."""
    f = lambda n: np.linalg.norm(v / n + tp) - n
    lo, hi = 1e-3, 100.0
    for _ in range(80):
        mid = 0.5 * (lo + hi)
        lo, hi = (mid, hi) if f(mid) > 0 else (lo, mid)
    return v / (0.5 * (lo + hi))


def sl1_branch_case(group, radius=0.06, seed=0):
    """Twelve labelled rows whose errors of channel ``group`` (0 centre, 1 axis, 2 theta, 3 score) sit at SL1_TARGETS, obtained
    by solving for reg given label, centre and template: in row j the channel j % width of the group is, in float32, EXACTLY
    SL1_TARGETS[j] when that is prev(1), 1 or next(1) (a search over the float32 neighbours of the solution, with new labels
    until one hits) and the other channels of the group sit at SL1_TARGETS[(j + 4 k) % 12] to 1e-6, so that quadratic and
    linear channels mix in one row (the gdot cross term of the axis gradient).  -> cls, reg, centre, tmpl, label,
    target (12, 10) float32 (nan outside the group), exact (12, 10) bool."""
    chans = SL1_GROUPS[group]
    A = 4
    rng = np.random.default_rng(7000 + 10 * group + seed)
    cls, reg, centre, tmpl, label = stage2_case(12, A, 7100 + group + seed, labelled=1.0)
    target = np.full((12, 10), np.nan, dtype=f32)
    exact = np.zeros((12, 10), dtype=bool)
    steps = np.arange(-48, 49)
    for j in range(12):
        main = chans[j % len(chans)]
        want = {ch: SL1_TARGETS[(j + 4 * ((ch - main) % len(chans))) % 12] for ch in chans}
        for attempt in range(400):
            c, gt = centre[j, :3], label[j, :10]
            a = int(np.argmin(anchor_similarity_32(tmpl, gt[None, 3:6])[0]))
            tp = tmpl[a]
            g = reg[j, a].copy()
            if group == 1:
                v = (gt[3:6] - tp[:3]).astype(f64) + np.array([want[ch] for ch in chans], dtype=f64)
                g[3:6] = _solve_axis(v, tp[:3].astype(f64)).astype(f32)
            else:
                zero = np.zeros(10, dtype=f32)
                base = -stage2_errors_32(zero, c, tp, gt, radius)          # the targets (gt - a) / scale, float32
                for ch in chans:
                    g[ch] = f32(f64(base[ch]) + f64(want[ch]))
            # the float32 neighbours of the main channel's solution: which of them lands on the target exactly?
            cand = np.repeat(g[None, :], len(steps), axis=0)
            cand[:, main] = nudge(g[main], steps)
            e = stage2_errors_32(cand, c[None], tp[None], gt[None], radius)
            hit = np.nonzero(e[:, main] == want[main])[0]
            if len(hit) or not SL1_BOUNDARY[j]:
                if len(hit):
                    g = cand[hit[np.argmin(np.abs(steps[hit]))]]
                    exact[j, main] = True
                reg[j, a] = g
                for ch in chans:
                    target[j, ch] = want[ch]
                break
            fresh = random_labels(rng, 1, centre[j:j + 1])[0]                # another label, same centre
            label[j, :10] = fresh
        else:
            raise RuntimeError("no float32 solution for row %d of group %d" % (j, group))
    return cls, reg, centre, tmpl, label, target, exact


def tied_logits_case(A, seed=0):
    """(rows, A) class scores with ties and the tie set of every row: the maximum at the first and the last anchor, in the
    middle and at the end, all equal, at the last two, and no tie.  -> cls, list of tied index tuples."""
    rng = np.random.default_rng(7200 + A + seed)
    last, mid = A - 1, A // 2
    sets = [(0, last), (mid, last), tuple(range(A)), (max(last - 1, 0), last), (0, mid), (int(rng.integers(0, A)),)]
    sets = [tuple(sorted(set(s))) for s in sets]
    cls = rng.normal(0, 1, (len(sets), A)).astype(f32)
    for i, s in enumerate(sets):
        cls[i, list(s)] = cls[i].max() + f32(0.5)
    return cls, sets


# label axes and the template ties they make: (axis, tie set among the four templates)
_E = f32(2.0 ** -10)
TIE_AXES = [((1, 0, 0), (0, 1, 2, 3)), ((0, 1, 0), (0, 1)), ((0, 0, 1), (0, 3)),
            ((1, _E, _E), (0,)), ((1, _E, -_E), (1,)), ((1, -_E, -_E), (2,)), ((1, -_E, _E), (3,)),
            ((0, 1, _E), (0,)), ((0, 1, -_E), (1,)), ((_E, 0, 1), (0, 3)), ((0, _E, 1), (0,)), ((0, -_E, 1), (3,)),
            ((0, 0, 0), (0, 1, 2, 3))]                                        # (zero axis: every 1 - cos is 1, the 1e-12 guard)


def tie_axes_case(seed=0):
    """One labelled row per entry of TIE_AXES (A = 4, the network's templates) -> cls, reg, centre, tmpl, label, tie sets."""
    n = len(TIE_AXES)
    cls, reg, centre, tmpl, label = stage2_case(n, 4, 7300 + seed, labelled=1.0)
    for i, (axis, _) in enumerate(TIE_AXES):
        label[i, 3:6] = np.asarray(axis, dtype=f32)
    return cls, reg, centre, tmpl, label, [t for _, t in TIE_AXES]


def guard_case(seed=0):
    """Rows that reach the 1e-12 guards: a zero label axis (row 0), reg[3:6] + template == 0 at the arg-max anchor (row 1), at
    the label's anchor (row 2) and at both (row 3)."""
    cls, reg, centre, tmpl, label = stage2_case(4, 4, 7400 + seed, labelled=1.0)
    label[0, 3:6] = 0
    g8 = np.argmin(anchor_similarity_32(tmpl, label[:, 3:6]), axis=1)
    for i in (1, 2, 3):
        other = (g8[i] + 1) % 4
        cls[i] = -1
        cls[i, other if i < 3 else g8[i]] = 2
        if i in (1, 3):
            reg[i, other if i == 1 else g8[i], 3:6] = -tmpl[other if i == 1 else g8[i], :3]
        if i in (2, 3):
            reg[i, g8[i], 3:6] = -tmpl[g8[i], :3]
    return cls, reg, centre, tmpl, label


def refine_case(m, seed, grasp_ld=10, label_ld=10):
    """Random refine inputs (about half of the rows label-positive) -> grasp (m,grasp_ld), cls (m,2), reg (m,10), label."""
    rng = np.random.default_rng(seed)
    label = np.full((m, label_ld), 3.0, dtype=f32)
    label[:, :10] = random_labels(rng, m, rng.normal(0, 0.2, (m, 3)).astype(f32))
    grasp = np.full((m, grasp_ld), -3.0, dtype=f32)
    grasp[:, :10] = label[:, :10]
    far = rng.uniform(0, 1, m) < 0.5
    grasp[far, :3] += f32(0.05)
    grasp[:, :3] += rng.normal(0, 0.004, (m, 3)).astype(f32)
    ax = grasp[:, 3:6] + rng.normal(0, 0.2, (m, 3)).astype(f32)
    grasp[:, 3:6] = ax / np.linalg.norm(ax, axis=1, keepdims=True)
    grasp[:, 6] += rng.normal(0, 0.3, m).astype(f32)
    return grasp, rng.normal(0, 1, (m, 2)).astype(f32), rng.normal(0, 0.5, (m, 10)).astype(f32), label


def _positive_rows(n, seed):
    """n refine rows that are label-positive with room to spare, class 1, kept."""
    grasp, cls, reg, label = refine_case(n, seed)
    grasp[:, :10] = label[:, :10]
    grasp[:, 0] += f32(0.004)
    grasp[:, 6] += f32(0.1)
    cls[:, 0], cls[:, 1] = -1, 1
    grasp[:, 7], reg[:, 7] = 0.5, 0.25
    return grasp, cls, reg, label


def refine_threshold_case(which, radius=0.06, score_thre=0.5, seed=0):
    """Three rows whose compared float32 value lands BELOW, ON and ABOVE its threshold by one float32 step, found by searching
    the float32 neighbours of a solution (the other conditions hold with room to spare):
      "near"    sqrtf(d2) against 0.025f            "aligned"  1 - cos against 0.5f: ON needs the quotient 0.5 exactly; below
      "angle"   |dtheta| against 1.047f             0.5 the quotient's spacing is 2^-24 and 1 - q is exact, so the closest value
      "score"   final[7] against score_thre         that 1 - q takes below 0.5 is 0.5 - 2^-24 (prev(0.5) = 0.5 - 2^-25 is not one)
      "class"   cls1 against cls0: below, equal, above
    -> grasp, cls, reg, label, wanted (3) float32 values of the compared quantity."""
    grasp, cls, reg, label = _positive_rows(3, 7500 + seed)
    rng = np.random.default_rng(7600 + seed)
    steps = np.arange(-200, 201)
    if which == "near":
        want = nudge(NEAR_T, [-1, 0, 1])
        for i in range(3):
            label[i, :3] = rng.uniform(-0.003, 0.003, 3)                  # small coordinates: fine float32 steps
            direction = unit_rows(rng, 1)[0].astype(f64)
            base = (label[i, :3].astype(f64) + direction * f64(NEAR_T)).astype(f32)
            g = np.repeat(np.repeat(base[None, None, :], len(steps), 0), 9, 1)
            g[:, :, 0] = nudge(base[0], steps)[:, None]
            g[:, :, 1] = nudge(base[1], np.arange(-4, 5))[None, :]
            off = g - label[i, :3]
            d = np.sqrt((off[..., 0] * off[..., 0] + off[..., 1] * off[..., 1]) + off[..., 2] * off[..., 2])
            hit = np.argwhere(d == want[i])
            grasp[i, :3] = g[tuple(hit[0])]
    elif which == "aligned":
        want = np.array([f32(0.5) - f32(2.0 ** -24), 0.5, nudge(f32(0.5), 1)], dtype=f32)
        for i in range(3):
            for attempt in range(200):
                a = label[i, 3:6].astype(f64)
                p = np.cross(a, unit_rows(rng, 1)[0].astype(f64))
                p /= np.linalg.norm(p)
                base = (0.5 * a + np.sqrt(0.75) * p).astype(f32)              # 60 degrees from the label's axis
                g = np.repeat(np.repeat(base[None, None, :], len(steps), 0), 41, 1)
                g[:, :, 0] = nudge(base[0], steps)[:, None]
                g[:, :, 1] = nudge(base[1], np.arange(-20, 21))[None, :]
                hit = np.argwhere(one_minus_cos_32(g, label[i, 3:6]) == want[i])
                if len(hit):
                    grasp[i, 3:6] = g[tuple(hit[0])]
                    break
                label[i, 3:6] = np.abs(unit_rows(rng, 1)[0])
            else:
                raise RuntimeError("no float32 axis pair with 1 - cos == %r" % want[i])
    elif which == "angle":
        want = nudge(ANGLE_T, [-1, 0, 1])
        for i in range(3):
            for attempt in range(200):
                sign = f32(1 if i != 1 else -1)
                cand = nudge(f32(label[i, 6] + sign * want[i]), np.arange(-8, 9))
                hit = np.nonzero(np.abs(cand - label[i, 6]) == want[i])[0]
                if len(hit):
                    grasp[i, 6] = cand[hit[0]]
                    break
                label[i, 6] = f32(rng.normal(0, 0.8))
            else:
                raise RuntimeError("no float32 angle pair")
    elif which == "score":
        want = nudge(f32(score_thre), [-1, 0, 1])
        for i in range(3):
            grasp[i, 7] = f32(score_thre) * f32(0.5)
            cand = nudge(f32(want[i] - grasp[i, 7]), np.arange(-8, 9))
            hit = np.nonzero(grasp[i, 7] + cand == want[i])[0]
            reg[i, 7] = cand[hit[0]]
    elif which == "class":
        cls[:, 0] = f32(0.3)
        cls[:, 1] = want = nudge(f32(0.3), [-1, 0, 1])
    else:
        raise ValueError(which)
    return grasp, cls, reg, label, np.asarray(want, dtype=f32)


REFINE_THRESHOLDS = ("near", "aligned", "angle", "score", "class")


def refine_branch_case(branch, seed=0):
    """Inputs for the host branches of region_losses.refine_loss: "no_positive", "no_negative", "no_class1", "none_kept" (class-1
    rows, none above the score threshold), "mixed".  48 rows."""
    grasp, cls, reg, label = refine_case(48, 7700 + seed)
    if branch == "no_positive":
        grasp[:, 0] += f32(0.1)
    elif branch == "no_negative":
        grasp[:, :7] = label[:, :7]
        grasp[:, 1] += f32(0.003)
    elif branch == "no_class1":
        cls[:, 0] = np.abs(cls[:, 0]) + 1
        cls[:, 1] = -1
    elif branch == "none_kept":
        grasp[:, 7] = np.minimum(grasp[:, 7], f32(0.2))
        reg[:, 7] = -np.abs(reg[:, 7])
    elif branch != "mixed":
        raise ValueError(branch)
    return grasp, cls, reg, label


def empty_class_case(empty, seed=0):
    """Stage-2 inputs (A = 4, 2 x 24 centres) whose labels' axes avoid the templates in ``empty``: those anchor classes are
    empty and ``per_class`` falls back to 1 when the smallest class is empty.  -> cls, reg, centre, tmpl, ground (2,24,10)."""
    n = 48
    cls, reg, centre, tmpl, label = stage2_case(n, 4, 7800 + seed + 10 * len(empty), labelled=0.85)
    rng = np.random.default_rng(7900 + seed)
    allowed = [a for a in range(4) if a not in empty]
    has = label[:, -1] != -1
    for i in np.nonzero(has)[0]:
        a = allowed[int(rng.integers(0, len(allowed)))]
        axis = TEMPLATES[a, :3] + rng.normal(0, 0.1, 3).astype(f32)
        label[i, 3:6] = axis / np.linalg.norm(axis)
    return cls, reg, centre, tmpl, label.reshape(2, n // 2, 10)


# ---- label matching ------------------------------------------------------------------------------------------------------------
def random_frames(rng, G, near):
    """G packed grasp records (G, 19): a random rotation [x | y | z] and a contact point beside a row of ``near`` (k, 3)."""
    q, _ = np.linalg.qr(rng.normal(0, 1, (G, 3, 3)))
    rec = np.zeros((G, 19), dtype=f32)
    frame = np.zeros((G, 4, 4), dtype=f32)
    frame[:, :3, :3] = q
    frame[:, :3, 3] = near[rng.integers(0, len(near), G)] + rng.normal(0, 0.01, (G, 3))
    frame[:, 3, 3] = 1
    rec[:, :16] = frame.reshape(G, 16)
    rec[:, 16:19] = rng.uniform(0, 1, (G, 3))
    return rec


def label_case(gcounts, Nc, seed, pad=7):
    """Scenes with ``gcounts`` grasps each, padded to Gmax = max + pad with records that sit EXACTLY on the scene's centres (a
    kernel that read past gcount would match them).  Centres: Nc rows of 6 channels; the first is far from every grasp.
    -> packed (B,Gmax,19), gcount (B) int32, centre (B,Nc,6)."""
    rng = np.random.default_rng(seed)
    B = len(gcounts)
    Gmax = max(gcounts) + pad
    centre = rng.normal(0, 0.2, (B, Nc, 6)).astype(f32)
    packed = np.zeros((B, Gmax, 19), dtype=f32)
    for b, G in enumerate(gcounts):
        packed[b] = random_frames(rng, Gmax, centre[b, :, :3])
        packed[b][G:, [3, 7, 11]] = centre[b, rng.integers(0, Nc, Gmax - G), :3]
        packed[b][G:, [0, 4, 8]] = 0
    centre[:, 0, :3] += 1.0
    return packed, np.asarray(gcounts, dtype=np.int32), centre


def duplicate_case(offset, seed=0):
    """One scene of 130 grasps in which grasps g and g + offset (offset 1: neighbouring lanes, 64: the same lane's next trip)
    share the contact point of a centre exactly, for g in (3, 40, 65) and centres 1, 2, 3; the later copy differs in every
    other column.  -> packed, gcount, centre, the (centre, first, second) triples."""
    packed, gcount, centre = label_case([130], 5, 8000 + offset + seed)
    triples = []
    for c, g in zip((1, 2, 3), (3, 40, 65)):
        packed[0, g, [3, 7, 11]] = centre[0, c, :3]
        packed[0, g, [0, 4, 8]] = 0                                 # no approach shift: the contact point is the centre
        packed[0, g + offset] = packed[0, g] * f32(-1)
        packed[0, g + offset, [3, 7, 11]] = packed[0, g, [3, 7, 11]]
        packed[0, g + offset, [0, 4, 8]] = 0
        triples.append((c, g, g + offset))
    return packed, gcount, centre, triples


def negative_distance_case(seed=0):
    """One scene, three centres one float32 step per coordinate away from the contact point of a grasp, at coordinates where the
    float32 expansion of that (tiny) squared distance comes out below zero.  -> packed, gcount, centre, the float32 distances."""
    rng = np.random.default_rng(8100 + seed)
    pts = rng.uniform(-1, 1, (4000, 3)).astype(f32)
    cps = nudge(pts, rng.integers(-1, 2, pts.shape))
    d = np.array([match_distance_32(p, q[None])[0] for p, q in zip(pts, cps)])
    pick = np.nonzero(d < 0)[0][:3]
    packed, gcount, centre = label_case([20], 3, 8101 + seed)
    centre[0, :, :3] = pts[pick]
    for c in range(3):
        packed[0, 5 + c, [3, 7, 11]] = cps[pick[c]]
        packed[0, 5 + c, [0, 4, 8]] = 0
    return packed, gcount, centre, d[pick]


# frames that send theta through the wrap steps: (x_z, z_z, y_x, what happens)
WRAP_FRAMES = [
    (0.6, 0.8, 0.5, "no flip, no wrap"),
    (0.6, 0.8, -0.5, "flip, pi - a inside (0, pi)"),
    (-0.6, 0.8, -0.5, "flip, pi + |a| > pi: third step"),
    (-0.0, -1.0, -0.5, "flip, a = -pi: 2 pi, first step, to 0"),
    (-0.0, -1.0, 0.5, "a = -pi: fourth step, to pi"),
    (0.0, -1.0, 0.5, "a = pi: stays (the third step is strict)"),
    (0.0, 1.0, -0.5, "flip, a = 0: pi, stays"),
    (0.6, 0.8, 0.0, "y_x = +0: no flip"),
    (0.6, 0.8, -0.0, "y_x = -0: no flip"),
    (-1e-3, -1.0, -1e-3, "flip, a just above -pi: third step"),
    (1.0, 0.0, -0.5, "flip, a = pi / 2"),
]
# (the second step, theta <= -2 pi, cannot be reached: atan2 lies in [-pi, pi] and a flipped angle in [0, 2 pi];
#  ``wrap_theta`` itself is exercised on that line by tests/test_loss_reference_cpu.py)


def wrap_case(seed=0):
    """One scene with one grasp per entry of WRAP_FRAMES (+ one whose x column is all -1: ``missing``) and one centre on each
    grasp's contact point.  -> packed, gcount, centre."""
    n = len(WRAP_FRAMES) + 1
    packed, gcount, centre = label_case([n], n, 8200 + seed, pad=2)
    centre[0, :, :3] = np.random.default_rng(8201 + seed).normal(0, 0.3, (n, 3))
    for i in range(n):
        packed[0, i, [3, 7, 11]] = centre[0, i, :3]
        packed[0, i, [0, 4, 8]] = 0
        if i < len(WRAP_FRAMES):
            xz, zz, yx, _ = WRAP_FRAMES[i]
            packed[0, i, 8], packed[0, i, 10], packed[0, i, 1] = f32(xz), f32(zz), f32(yx)
        else:
            packed[0, i, [0, 4, 8]] = -1
            centre[0, i, :3] = contact_points_32(packed[0, i], 0.06)
    centre[0, :len(WRAP_FRAMES), :3] = contact_points_32(packed[0, :len(WRAP_FRAMES)], 0.06)
    return packed, gcount, centre


# (gcounts, Nc, seed) of the random-bulk label comparisons: tests/test_loss_reference_cpu.py asserts that each skips at most 1 %
# of its rows at a wrap line.  The last four are the launch edges: no grasp, one, one short of / exactly / one past a full trip of
# the 64 lanes, two trips and two more lanes; B * Nc = 6 Nc is no multiple of 4
LABEL_BULK = [([130, 65, 64, 63, 1], 9, 11), ([70, 40, 200], 5, 12)] + [([0, 1, 63, 64, 65, 130], Nc, 30 + Nc) for Nc in (1, 3, 5, 9)]


def max_sq_case(seed=0):
    """One scene of 40 grasps and four centres, and the limits that sit below, ON and above the float32 distance of centre 1
    to its nearest grasp (compared as float64: the neighbours are float64 neighbours).  -> packed, gcount, centre, the distance,
    [(max_sq, whether centre 1 keeps its grasp)]: the comparison is inclusive."""
    packed, gcount, centre = label_case([40], 4, 21 + seed)
    d = label_match(packed, gcount, centre, 0.06, np.inf)["best"][0, 1]
    return packed, gcount, centre, d, [(np.nextafter(d, -np.inf), False), (d, True), (np.nextafter(d, np.inf), True)]


def theta_tolerance(res, atan_error):
    """The bound of a float32 theta against ``res["theta"]``: twice the worst error ``atan_error`` measured for a float32 atan2
    on the same arguments, one ulp of the result, and one rounding of magnitude ``theta_mag`` per addition made (the flip and
    the wrap steps)."""
    return 2.0 * atan_error + ulp32(res["theta"]) + res["theta_adds"] * U * res["theta_mag"]
