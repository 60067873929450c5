"""The loss and label kernels (csrc/losses.hip) on the MI355X through their C entry points, against the float64 restatement of
their contract (tests/loss_reference.py, whose builders tests/test_loss_reference_cpu.py has shown to hold their cases): ties,
thresholds, smooth-L1 on both sides of |e| = 1, the rows / leading-dimension / block edges with sentinel-filled outputs, the
label matching at G = 0 ... 130 with duplicates, an inclusive limit and every reachable wrap step, the host branches of
region_losses with FUSED on and off, and the rejected shapes.

Decisions (pick, g8, terms[8], the refine flags and terms[16..19], the matched grasp, has / flip / missing / wide_row and every
label column but theta) are compared exactly.  Values are compared within ``k 2^-24 magnitude`` with the k counted in
loss_reference.  The three library functions get a measured allowance, never taken from the kernel's own output:
  cross entropy   the float32 additions around expf / logf are counted like any other (loss: ``+ mx`` and ``- x[tg]``, 2
                  roundings of magnitude |mx| + |log se| + |x_tg|, and A - 1 additions in se; dcls: the argument x - lse carries
                  3 roundings of its magnitude and those A - 1, which expf turns into a relative error, then ``- onehot`` and
                  ``* scale``); on top of that twice the worst error of torch's float32 log_softmax (relative to the same
                  magnitude) resp. softmax (absolute) on the same rows against float64, plus one ulp of the result.
  theta           twice the worst error of torch's float32 atan2 on the same arguments, one ulp of the result and one
                  rounding per addition made (``ref.theta_tolerance``).
Every test prints the worst observed fraction of its bound and torch's baselines (``pytest -s``: ``bound-fraction``, ``torch
baseline``), and for the cross entropy also the fraction of twice torch's error plus one ulp alone, without the counted
additions (``uncounted-fraction``, not asserted).

Measured on the MI355X, worst fraction of the bound over every case of this file (48 cases, 5.3 s, the slowest 0.9 s):
  stage-2 rows     next_grasp 0.82, terms 0.57, dreg 0.80; smooth-L1 branch rows terms 0.34, dreg 0.68; ties and guards <= 0.74
  refine rows      final 0.995 (final[3:] is one correctly rounded addition: half an ulp can reach the whole bound), terms 0.52,
                   dreg 0.65
  cross entropy    loss 0.22, dcls 0.20; without the counted additions loss 0.42 and dcls 3.8 at nb >= 64 (``expf(x - lse)`` rounds
                   lse at the size of the logits, torch's ``exp(x - max) / sum`` does not), 22.5 / 24.3 at nb = 1, where the
                   baseline is one row on which torch is exact
  theta            bulk 0.35, duplicates 0.18, limit 0.23, padding 0.30, wrap cases 0.16
  region_losses    fused path against the reference: final 0.999, values 0.02, ce 0.04, dreg 0.70, dcls 0.24
Torch's float32 baselines on the same inputs: log_softmax <= 1.85 x 2^-24 of |max| + |log sum| + |x_target|, softmax <= 1.61 x
2^-24 absolute, atan2 <= 0.27 x 2^-24 pi.
"""
import ctypes

import numpy as np
import pytest
import torch

from . import loss_reference as ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENT = -777.0
RADIUS = float(np.float32(0.06))
THRE = 0.5
DEPTH = float(np.float32(0.06))
MAX_SQ = 0.005
OK, ERR_SHAPE, ERR_UNSUPPORTED = 0, -1, -3


@pytest.fixture(scope="module")
def L():
    from regnet_for_3d_grasping_amd import _lib
    return _lib.lib


@pytest.fixture(scope="module")
def net():
    from regnet_for_3d_grasping_amd.gripper_region_network import GripperRegionNetwork
    return GripperRegionNetwork(training=True, group_num=256, gripper_num=64, grasp_score_threshold=THRE, radius=RADIUS,
                                reg_channel=10).to(DEV)


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def full(shape, dtype=torch.float32, value=SENT):
    return torch.full(shape, value, dtype=dtype, device=DEV)


def stream():
    return torch.cuda.current_stream(torch.device(DEV)).cuda_stream


def host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def within(name, got, want, bound):
    """|got - want| <= bound everywhere (bound 0: equal); prints the worst fraction of the bound used."""
    got, want, bound = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64), np.asarray(bound, dtype=np.float64)
    assert got.shape == want.shape, (name, got.shape, want.shape)
    err = np.abs(got - want)
    assert np.isfinite(got).all(), name
    frac = np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err > 0, np.inf, 0.0))
    worst = float(frac.max()) if frac.size else 0.0
    print("bound-fraction %-28s %.3f" % (name, worst))
    assert worst <= 1.0, (name, worst, float(err.max()))


# ---- stage-2 rows ------------------------------------------------------------------------------------------------------------
def run_stage2(L, cls, reg, centre, tmpl, label, weights, rows, pad=3):
    n, A = cls.shape
    m = n if rows is None else len(rows)
    t = [dev(x) for x in (cls, reg, centre, tmpl, label)]
    rows_t = None if rows is None else dev(np.asarray(rows, dtype=np.int64))
    w = (ctypes.c_float * 4)(*[float(x) for x in weights])
    M = m + pad
    out = dict(next_grasp=full((M, 10)), pick=full((M,), torch.int32, -7), g8=full((M,), torch.int32, -7), a_gt=full((M, 7)),
               terms=full((M, 12)), dreg=full((n, A, 10)))
    status = L.regnet_stage2_loss_rows_f32(t[0].data_ptr(), t[1].data_ptr(), A, 10, t[2].data_ptr(), centre.shape[1],
                                           t[3].data_ptr(), t[4].data_ptr(), label.shape[1], RADIUS, ctypes.addressof(w),
                                           None if rows_t is None else rows_t.data_ptr(), m, out["next_grasp"].data_ptr(),
                                           out["pick"].data_ptr(), out["g8"].data_ptr(), out["a_gt"].data_ptr(),
                                           out["terms"].data_ptr(), out["dreg"].data_ptr(), stream())
    assert status == OK
    return {k: host(v) for k, v in out.items()}


def check_stage2(tag, got, want, n, A):
    rows, m = want["rows"], len(want["rows"])
    for key in ("next_grasp", "a_gt", "terms"):
        assert (got[key][m:] == np.float32(SENT)).all(), (tag, key, "written past m")
    assert (got["pick"][m:] == -7).all() and (got["g8"][m:] == -7).all()
    assert np.array_equal(got["pick"][:m], want["pick"]), (tag, "pick: first maximum")
    assert np.array_equal(got["g8"][:m], want["g8"]), (tag, "g8: first minimum")
    assert np.array_equal(got["a_gt"][:m], want["a_gt"])
    assert np.array_equal(got["terms"][:m, 8], want["equal"].astype(np.float32)) and (got["terms"][:m, 9:] == 0).all()
    within(tag + " next_grasp", got["next_grasp"][:m], want["next_grasp"].val, want["next_grasp"].bound)
    within(tag + " terms", got["terms"][:m], want["terms"].val, want["terms"].bound)
    untouched = np.ones(n, dtype=bool)
    untouched[rows] = False
    assert (got["dreg"][untouched] == np.float32(SENT)).all(), (tag, "dreg of a row that is not in rows")
    other = np.ones((m, A), dtype=bool)
    other[np.arange(m), want["g8"]] = False
    assert (got["dreg"][rows][other] == 0).all(), (tag, "dreg of the anchors other than g8")
    d = got["dreg"][rows, want["g8"]]
    within(tag + " dreg", d, want["dreg"].val, want["dreg"].bound)
    lin = want["dreg32_linear"]
    assert np.array_equal(d[~np.isnan(lin)], lin[~np.isnan(lin)]), (tag, "+-w on the linear side of smooth-L1")


S2_WEIGHTS = np.array([10.0 / 21, 5.0 / 21, 1.0 / 7, 1.0 / 21], dtype=np.float32)


@pytest.mark.parametrize("A", [1, 4, 8, 64])
def test_stage2_rows_shapes_rows_and_leading_dimensions(L, A):
    for m in (1, 63, 64, 65, 130):
        for mode in ("all", "subset", "unordered"):
            n = m if mode == "all" else m + 9
            wide = mode != "subset"
            cls, reg, centre, tmpl, label = ref.stage2_case(n, A, 100 * A + m, labelled=0.8, centre_ld=6 if wide else 3,
                                                            label_ld=13 if wide else 10, spread=1.5 if m % 2 else 0.3)
            rng = np.random.default_rng(m + A)
            rows = None if mode == "all" else np.sort(rng.permutation(n)[:m]) if mode == "subset" else rng.permutation(n)[:m]
            want = ref.stage2_rows(cls, reg, centre, tmpl, label, RADIUS, S2_WEIGHTS, rows)
            got = run_stage2(L, cls, reg, centre, tmpl, label, S2_WEIGHTS, rows)
            check_stage2("stage2 A=%d m=%d %s" % (A, m, mode), got, want, n, A)


@pytest.mark.parametrize("group", [0, 1, 2, 3])
def test_stage2_smooth_l1_on_both_sides_of_one(L, group):
    cls, reg, centre, tmpl, label, target, exact = ref.sl1_branch_case(group)
    want = ref.stage2_rows(cls, reg, centre, tmpl, label, RADIUS, S2_WEIGHTS)
    got = run_stage2(L, cls, reg, centre, tmpl, label, S2_WEIGHTS, None)
    check_stage2("sl1 group %d" % group, got, want, 12, 4)
    lin = want["dreg32_linear"]
    chans = list(ref.SL1_GROUPS[group])
    if group != 1:
        assert (~np.isnan(lin[:, chans])).sum() >= 6            # |e| = 1, next(1) and 3 of both signs: exactly +-w
        d = got["dreg"][np.arange(12), want["g8"]]
        e = want["e32"]
        quad = np.abs(e[:, chans]) < 1                          # prev(1) is still quadratic: w * e, not w
        w = S2_WEIGHTS[group]
        assert np.array_equal(d[:, chans][quad], (w * e[:, chans])[quad])


@pytest.mark.parametrize("A", [1, 2, 4, 8, 64])
def test_stage2_pick_is_the_first_maximum_on_tied_scores(L, A):
    tied, sets = ref.tied_logits_case(A)
    n = len(sets)
    cls, reg, centre, tmpl, label = ref.stage2_case(n, A, 300 + A, labelled=1.0)
    want = ref.stage2_rows(tied, reg, centre, tmpl, label, RADIUS, S2_WEIGHTS)
    assert want["pick"].tolist() == [s[0] for s in sets]
    check_stage2("tied scores A=%d" % A, run_stage2(L, tied, reg, centre, tmpl, label, S2_WEIGHTS, None), want, n, A)


def test_stage2_g8_is_the_first_minimum_on_axis_aligned_labels_and_guards(L):
    cls, reg, centre, tmpl, label, sets = ref.tie_axes_case()
    want = ref.stage2_rows(cls, reg, centre, tmpl, label, RADIUS, S2_WEIGHTS)
    assert want["g8"].tolist() == [s[0] for s in sets]
    check_stage2("tie axes", run_stage2(L, cls, reg, centre, tmpl, label, S2_WEIGHTS, None), want, len(sets), 4)
    cls, reg, centre, tmpl, label = ref.guard_case()
    want = ref.stage2_rows(cls, reg, centre, tmpl, label, RADIUS, S2_WEIGHTS)
    got = run_stage2(L, cls, reg, centre, tmpl, label, S2_WEIGHTS, None)
    check_stage2("1e-12 guards", got, want, 4, 4)
    assert (got["next_grasp"][[1, 3], 3:6] == 0).all()


def test_fused_and_tensor_paths_pick_the_same_anchor_on_axis_aligned_labels(net):
    """The labels that axis-aligned objects produce tie two or four templates: the kernel takes the first minimum, and the
    tensor path (a stable sort) must take the same one."""
    from regnet_for_3d_grasping_amd import region_losses
    cls, reg, centre, tmpl, label, sets = ref.tie_axes_case()
    ground = dev(label).view(1, -1, 10)
    np.random.seed(5)
    fused = region_losses.stage2_loss(dev(reg), dev(cls), dev(centre), dev(tmpl), ground, RADIUS)
    old, region_losses.FUSED = region_losses.FUSED, False
    try:
        np.random.seed(5)
        plain = net.compute_loss(dev(reg), net._enumerate_anchors(dev(centre)), dev(cls), ground)
    finally:
        region_losses.FUSED = old
    first = tmpl[[s[0] for s in sets]]
    assert np.array_equal(host(fused[4])[:, 3:], first), "fused: first minimum"
    assert np.array_equal(host(plain[4])[:, 3:], first), "tensor path: first minimum"
    for x, y in zip(fused[1], plain[1]):
        assert torch.allclose(x.detach().float().cpu(), y.detach().float().cpu(), rtol=1e-5, atol=2e-6)


# ---- cross-entropy rows ------------------------------------------------------------------------------------------------------
def ce_inputs(A, n, seed):
    rng = np.random.default_rng(seed)
    cls = rng.normal(0, 2, (n, A)).astype(np.float32)
    cls[0] = np.where(np.arange(A) % 2 == 0, 80, -80)
    cls[1] = np.linspace(-5e3, 5e3, A) if A > 1 else 1e4              # spread 1e4
    cls[2] = 80
    cls[3] = -80
    cls[4, :] = rng.normal(0, 30, A)
    return cls


def ce_tolerances(cls_rows, tg, scale, loss64, soft64):
    """-> (tolerance of the loss (nb), of dcls (nb, A), torch's measured baselines, the same two tolerances without the counted
    additions: twice torch's worst error on these rows plus one ulp of the result, printed beside the asserted ones)."""
    nb, A = cls_rows.shape
    x = cls_rows.astype(np.float64)
    mx = x.max(axis=1)
    logse = np.log(np.exp(x - mx[:, None]).sum(axis=1))
    ar = np.arange(nb)
    mag = np.abs(mx) + np.abs(logse) + np.abs(x[ar, tg])
    xt = dev(cls_rows)
    ls32 = host(torch.log_softmax(xt, dim=1)).astype(np.float64)
    sm32 = host(torch.softmax(xt, dim=1)).astype(np.float64)
    e_ls = float((np.abs(-ls32[ar, tg] - loss64) / mag).max())
    e_sm = float(np.abs(sm32 - soft64).max())
    assert e_ls <= 8 * ref.U and e_sm <= 8 * ref.U               # (torch's own functions are good to a few roundings)
    tol_loss = (2 * ref.U + 2 * e_ls) * mag + (A - 1) * ref.U + ref.ulp32(loss64)
    mag_t = np.abs(x) + (np.abs(mx) + np.abs(logse))[:, None]
    onehot = np.zeros((nb, A))
    onehot[ar, tg] = 1
    s = float(np.float32(scale))
    tol_d = s * (soft64 * ref.U * (3 * mag_t + (A - 1)) + 2 * ref.U * (soft64 + onehot) + 2 * e_sm + ref.ulp32(soft64))
    plain_loss = 2 * e_ls * mag + ref.ulp32(loss64)
    plain_d = s * (2 * e_sm + ref.ulp32(soft64))
    return tol_loss, tol_d, e_ls, e_sm, plain_loss, plain_d


def run_ce(L, cls, target, idx, rows, scale, pad=3):
    n, A = cls.shape
    nb = len(idx)
    loss, dcls = full((nb + pad,)), torch.zeros((n, A), dtype=torch.float32, device=DEV)
    t = [dev(cls), dev(np.asarray(target, dtype=np.int32)), dev(np.asarray(idx, dtype=np.int64))]
    rows_t = None if rows is None else dev(np.asarray(rows, dtype=np.int64))
    status = L.regnet_ce_rows_f32(t[0].data_ptr(), A, t[1].data_ptr(), t[2].data_ptr(), None if rows is None else rows_t.data_ptr(),
                                  nb, float(scale), loss.data_ptr(), dcls.data_ptr(), stream())
    assert status == OK
    return host(loss), host(dcls)


@pytest.mark.parametrize("A", [1, 2, 8, 64])
def test_ce_rows_stable_log_sum_exp_targets_scale_and_untouched_rows(L, A):
    n = 100
    cls = ce_inputs(A, n, 400 + A)
    for nb in (1, 64, 65):
        for with_rows in (False, True):
            rng = np.random.default_rng(nb + A)
            rows = rng.permutation(np.concatenate([np.arange(5), 5 + rng.permutation(n - 5)[:75]])) if with_rows else None
            compact = 80 if with_rows else n
            row_of = np.arange(n) if rows is None else rows
            special = [int(np.nonzero(row_of == r)[0][0]) for r in range(5)]            # the +-80 / spread 1e4 rows first
            rest = np.array([j for j in rng.permutation(compact) if j not in special], dtype=np.int64)
            idx = np.concatenate([np.array(special, dtype=np.int64), rest])[:nb] if nb > 1 else np.array(special[:1], dtype=np.int64)
            target = np.where(np.arange(compact) % 2 == 0, np.argmax(cls[row_of], axis=1), np.argmin(cls[row_of], axis=1))
            scale = 1.0 / nb if nb > 1 else 0.37
            loss64, dcls64, drawn = ref.ce_rows(cls, target, idx, rows, scale)
            r = row_of[idx]
            soft64 = dcls64[r] / np.float64(np.float32(scale))
            soft64[np.arange(nb), target[idx]] += 1.0
            tol_loss, tol_d, e_ls, e_sm, plain_loss, plain_d = ce_tolerances(cls[r], target[idx], scale, loss64, soft64)
            print("torch baseline A=%d nb=%d: log_softmax %.2f x 2^-24 magnitude, softmax %.2f x 2^-24" % (A, nb, e_ls / ref.U, e_sm / ref.U))
            loss, dcls = run_ce(L, cls, target, idx, rows, scale)
            tag = "ce A=%d nb=%d rows=%s" % (A, nb, with_rows)
            assert (loss[nb:] == np.float32(SENT)).all(), "loss written past nb"
            assert (dcls[~drawn] == 0).all(), "dcls of a row that was not drawn"
            print("uncounted-fraction %-22s loss %.3f dcls %.3f" % (tag, float((np.abs(loss[:nb] - loss64) / plain_loss).max()),
                                                                     float((np.abs(dcls[r] - dcls64[r]) / plain_d).max())))
            within(tag + " loss", loss[:nb], loss64, tol_loss)
            within(tag + " dcls", dcls[r], dcls64[r], tol_d)


# ---- refine rows -------------------------------------------------------------------------------------------------------------
def run_refine(L, grasp, cls, reg, label, pad=3):
    m = reg.shape[0]
    t = [dev(x) for x in (grasp, cls, reg, label)]
    out = dict(final=full((m + pad, 10)), flags=full((3 * m + pad,), torch.uint8, 9), terms=full((m + pad, 20)),
               dreg=full((m + pad, 10)))
    status = L.regnet_refine_loss_rows_f32(t[0].data_ptr(), grasp.shape[1], t[1].data_ptr(), t[2].data_ptr(), t[3].data_ptr(),
                                           label.shape[1], 10, RADIUS, THRE, m, out["final"].data_ptr(), out["flags"].data_ptr(),
                                           out["terms"].data_ptr(), out["dreg"].data_ptr(), stream())
    assert status == OK
    return {k: host(v) for k, v in out.items()}


def check_refine(tag, got, want):
    m = want["flags"].shape[1]
    assert (got["flags"][3 * m:] == 9).all() and all((got[k][m:] == np.float32(SENT)).all() for k in ("final", "terms", "dreg"))
    assert np.array_equal(got["flags"][:3 * m].reshape(3, m), want["flags"]), (tag, "class / kept / positive flags")
    assert np.array_equal(got["terms"][:m, 16:20], want["terms"].val[:, 16:20].astype(np.float32)), (tag, "confusion counts")
    assert (got["dreg"][:m][~want["pos"]] == 0).all(), (tag, "dreg of a row that is not label-positive")
    within(tag + " final", got["final"][:m], want["final"].val, want["final"].bound)
    within(tag + " terms", got["terms"][:m], want["terms"].val, want["terms"].bound)
    within(tag + " dreg", got["dreg"][:m], want["dreg"].val, want["dreg"].bound)


@pytest.mark.parametrize("m", [1, 63, 64, 65, 130])
def test_refine_rows_shapes_and_leading_dimensions(L, m):
    grasp, cls, reg, label = ref.refine_case(m, 500 + m, grasp_ld=12, label_ld=13)
    want = ref.refine_rows(grasp, cls, reg, label, RADIUS, THRE)
    if m > 1:
        assert want["pos"].any() and not want["pos"].all() and want["one"].any() and not want["one"].all()
    check_refine("refine m=%d" % m, run_refine(L, grasp, cls, reg, label), want)


@pytest.mark.parametrize("which", ref.REFINE_THRESHOLDS)
def test_refine_decisions_on_and_beside_their_thresholds(L, which):
    grasp, cls, reg, label, _ = ref.refine_threshold_case(which, RADIUS, THRE)
    want = ref.refine_rows(grasp, cls, reg, label, RADIUS, THRE)
    expect = dict(near=("pos", [1, 0, 0]), aligned=("pos", [1, 0, 0]), angle=("pos", [1, 0, 0]), score=("kept", [0, 0, 1]),
                  **{"class": ("one", [0, 0, 1])})[which]
    assert want[expect[0]].astype(int).tolist() == expect[1]
    check_refine("refine threshold " + which, run_refine(L, grasp, cls, reg, label), want)


# ---- label matching ------------------------------------------------------------------------------------------------------------
def run_label(L, packed, gcount, centre, max_sq=MAX_SQ, pad=2):
    B, Nc = centre.shape[:2]
    Gmax = packed.shape[1]
    p, g = dev(packed), dev(np.asarray(gcount, dtype=np.int32))
    view = dev(centre)[:, :, :3]                                     # xyz of wider rows: the strides are passed
    assert view.stride(1) == centre.shape[2] and view.stride(2) == 1
    out, wide = full((B * Nc + pad, 10)), full((B * Nc + pad,), torch.int32, -7)
    status = L.regnet_label_match_f32(p.data_ptr(), g.data_ptr(), Gmax, view.data_ptr(), view.stride(0), view.stride(1), B, Nc,
                                      DEPTH, float(max_sq), out.data_ptr(), wide.data_ptr(), stream())
    assert status == OK
    out, wide = host(out), host(wide)
    assert (out[B * Nc:] == np.float32(SENT)).all() and (wide[B * Nc:] == -7).all(), "written past B * Nc"
    return out[:B * Nc].reshape(B, Nc, 10), wide[:B * Nc].reshape(B, Nc)


def check_label(tag, got, wide, want, skip_near_wrap=False):
    other = [0, 1, 2, 3, 4, 5, 7, 8, 9]
    assert np.array_equal(np.ascontiguousarray(got[..., other]).view(np.uint32),
                          np.ascontiguousarray(want["out"][..., other]).view(np.uint32)), (tag, "copied / negated columns")
    assert np.array_equal(wide, want["wide_row"]), (tag, "wide_row")
    filler = ~want["has"]
    assert (got[filler][:, 3:6] == 1).all() and (got[filler][:, [0, 1, 2, 6, 7, 8, 9]] == -1).all(), (tag, "filler rows")
    live = ~want["missing"]
    y, x = want["atan_y"][live], want["atan_x"][live]
    atan_error = 0.0
    if len(y):
        t32 = host(torch.atan2(dev(y), dev(x))).astype(np.float64)
        atan_error = float(np.abs(t32 - np.arctan2(y.astype(np.float64), x.astype(np.float64))).max())
        assert atan_error <= 4 * ref.U * np.pi
        print("torch baseline %s: atan2 %.2f x 2^-24 pi" % (tag, atan_error / (ref.U * np.pi)))
    keep = ~want["near_wrap"] if skip_near_wrap else np.ones(want["theta"].shape, dtype=bool)
    assert keep.mean() >= 0.99
    tol = np.where(want["missing"], 0.0, ref.theta_tolerance(want, atan_error))
    within(tag + " theta", got[..., 6][keep], want["theta"][keep], tol[keep])


@pytest.mark.parametrize("gcounts,Nc,seed", ref.LABEL_BULK)
def test_label_match_bulk_and_launch_edges(L, gcounts, Nc, seed):
    packed, gcount, centre = ref.label_case(gcounts, Nc, seed)
    packed[::2, :, 17] = -1                                          # scenes without an antipodal score: wide_row 0
    want = ref.label_match(packed, gcount, centre, DEPTH, MAX_SQ)
    got, wide = run_label(L, packed, gcount, centre)
    check_label("label %s Nc=%d" % (gcounts, Nc), got, wide, want, skip_near_wrap=True)


@pytest.mark.parametrize("offset", [1, 64])
def test_label_match_takes_the_lower_index_of_two_equal_distances(L, offset):
    packed, gcount, centre, triples = ref.duplicate_case(offset)
    want = ref.label_match(packed, gcount, centre, DEPTH, MAX_SQ)
    got, wide = run_label(L, packed, gcount, centre)
    for c, first, second in triples:
        assert want["index"][0, c] == first
        assert np.array_equal(got[0, c, 7:10], packed[0, first, 16:19]) and not np.array_equal(got[0, c, 7:10], packed[0, second, 16:19])
    check_label("duplicates +%d" % offset, got, wide, want)


def test_label_match_limit_is_inclusive_and_a_negative_distance_is_kept(L):
    packed, gcount, centre, d, limits = ref.max_sq_case()
    for max_sq, has in limits:
        want = ref.label_match(packed, gcount, centre, DEPTH, max_sq)
        assert bool(want["has"][0, 1]) == has
        got, wide = run_label(L, packed, gcount, centre, max_sq)
        assert (got[0, 1, 0] != -1) == has, ("distance %r, limit %r" % (d, max_sq))
        check_label("limit", got, wide, want)
    packed, gcount, centre, dist = ref.negative_distance_case()
    want = ref.label_match(packed, gcount, centre, DEPTH, MAX_SQ)
    assert (dist < 0).all() and want["has"].all()
    got, wide = run_label(L, packed, gcount, centre)
    check_label("negative distance", got, wide, want)


def test_label_match_reads_no_record_past_gcount(L):
    packed, gcount, centre = ref.label_case([0, 1, 63], 3, 22)
    want = ref.label_match(packed, gcount, centre, DEPTH, MAX_SQ)
    got, wide = run_label(L, packed, gcount, centre)
    check_label("padding", got, wide, want)
    assert (wide[0] == 0).all() and (got[0, :, 3:6] == 1).all()


def test_label_match_theta_in_every_wrap_branch(L):
    packed, gcount, centre = ref.wrap_case()
    want = ref.label_match(packed, gcount, centre, DEPTH, MAX_SQ)
    got, wide = run_label(L, packed, gcount, centre)
    check_label("wrap", got, wide, want)                            # (skips nothing)
    n = len(ref.WRAP_FRAMES)
    th, pi = got[0, :, 6], ref.PI32
    assert th[3] == 0 and th[4] == pi and th[5] == pi and th[6] == pi and th[n] == -1
    assert th[7] == th[0] and th[8] == th[0]                        # y_x = +0 and -0 do not flip
    assert got[0, 7, 3] == 0 and got[0, 8, 3] == 0 and np.signbit(got[0, 8, 3]) and not np.signbit(got[0, 7, 3])


# ---- the host branches of region_losses ------------------------------------------------------------------------------------------
def same(a, b):
    if a is None or b is None:
        assert a is None and b is None
        return
    a, b = a.detach().float().cpu(), b.detach().float().cpu()
    assert a.shape == b.shape and torch.allclose(a, b, rtol=1e-5, atol=2e-6, equal_nan=True), float((a - b).abs().max())


def ce_mean_tolerance(cls_rows, tg, res):
    nb = len(tg)
    soft = res["dcls_rows"] * nb
    soft[np.arange(nb), tg] += 1
    tol_loss, tol_d = ce_tolerances(cls_rows, tg, 1.0 / nb, res["ce_rows"], soft)[:2]
    return float(tol_loss.max() + (nb + 1) * ref.U * np.abs(res["ce_rows"]).mean()), tol_d


@pytest.mark.parametrize("empty", [(2,), (1, 3)])
def test_stage2_loss_with_empty_anchor_classes_fused_and_tensor_paths(net, empty):
    from regnet_for_3d_grasping_amd import region_losses
    cls, reg, centre, tmpl, ground = ref.empty_class_case(empty)
    np.random.seed(70)
    want = ref.stage2_loss(cls, reg, centre, tmpl, ground.reshape(-1, 10), RADIUS)
    after_ref = int(np.random.randint(0, 2 ** 31 - 1))
    assert want["per_class"] == 1 and want["nb"] == 4 - len(empty)
    outs = []
    for fused in (True, False):
        x_reg, x_cls = dev(reg).requires_grad_(True), dev(cls).requires_grad_(True)
        np.random.seed(70)
        old, region_losses.FUSED = region_losses.FUSED, fused
        try:
            if fused:
                res = region_losses.stage2_loss(x_reg, x_cls, dev(centre), dev(tmpl), dev(ground), RADIUS)
            else:
                res = net.compute_loss(x_reg, net._enumerate_anchors(dev(centre)), x_cls, dev(ground))
        finally:
            region_losses.FUSED = old
        assert int(np.random.randint(0, 2 ** 31 - 1)) == after_ref, "numpy stream position"
        res[1][0].backward()
        outs.append((res, x_reg.grad.clone(), x_cls.grad.clone()))
    (ra, gra, gca), (rb, grb, gcb) = outs
    same(ra[0], rb[0])
    for x, y in zip(ra[1] + ra[2], rb[1] + rb[2]):
        same(x, y)
    same(ra[3], rb[3]); same(ra[4], rb[4]); assert torch.equal(ra[5], rb[5])
    same(gra, grb); same(gca, gcb)
    # the fused path against the float64 reference
    v = want["values"]
    lt = [float(x) for x in ra[1]]
    r = want["rows"][want["idx"]]
    tg = want["rows_out"]["g8"][want["idx"]]
    ce_tol, tol_d = ce_mean_tolerance(cls[r], tg, dict(ce_rows=want["ce_rows"], dcls_rows=want["dcls"][r].copy()))
    within("host stage2 ce", lt[1], want["ce"], ce_tol)
    for j in range(8):
        within("host stage2 value %d" % j, lt[2 + j], v[j].val, v[j].bound)
    assert float(ra[2][0]) == v[8].val and float(ra[2][1]) == v[9].val
    total = want["reg_loss"].val + want["ce"]
    within("host stage2 loss", lt[0], total, want["reg_loss"].bound + ce_tol + ref.U * abs(total))
    within("host stage2 dreg", host(gra), want["dreg"], want["dreg_bound"])
    got_dcls = host(gca)
    assert (got_dcls[~want["drawn"]] == 0).all()
    within("host stage2 dcls", got_dcls[r], want["dcls"][r], tol_d)


@pytest.mark.parametrize("branch", ["no_positive", "no_negative", "no_class1", "none_kept", "mixed"])
def test_refine_loss_host_branches_fused_and_tensor_paths(net, branch):
    from regnet_for_3d_grasping_amd import region_losses
    grasp, cls, reg, label = ref.refine_branch_case(branch)
    np.random.seed(80)
    want = ref.refine_loss(grasp, cls, reg, label, RADIUS, THRE)
    after_ref = int(np.random.randint(0, 2 ** 31 - 1))
    outs = []
    for fused in (True, False):
        x_reg, x_cls = dev(reg).requires_grad_(True), dev(cls).requires_grad_(True)
        np.random.seed(80)
        old, region_losses.FUSED = region_losses.FUSED, fused
        try:
            res = net.compute_loss_refine(dev(grasp), x_cls, x_reg, dev(label))
        finally:
            region_losses.FUSED = old
        assert int(np.random.randint(0, 2 ** 31 - 1)) == after_ref, "numpy stream position"
        if res[5][0].requires_grad:
            res[5][0].backward()
        outs.append((res, x_reg.grad, x_cls.grad))
    (ra, gra, gca), (rb, grb, gcb) = outs
    for k in range(3):
        same(ra[k], rb[k])
    assert torch.equal(ra[3].cpu(), rb[3].cpu()) and torch.equal(ra[4].cpu(), rb[4].cpu())
    assert len(ra[5]) == len(rb[5]) == 18
    for x, y in zip(tuple(ra[5]) + tuple(ra[6]), tuple(rb[5]) + tuple(rb[6])):
        same(torch.as_tensor(x), torch.as_tensor(y))
    same(gra, grb); same(gca, gcb)
    # the fused path against the float64 reference
    assert np.array_equal(host(ra[3]), want["class_select"]) and np.array_equal(host(ra[4]), want["score_select"])
    final = want["rows_out"]["final"]
    within("host refine final", host(ra[0]), final.val[want["class_select"]], final.bound[want["class_select"]])
    lt = [float(x) for x in ra[5]]
    for j in range(16):
        if np.isnan(want["values"][j].val):
            assert np.isnan(lt[2 + j]) and branch == "none_kept" and j >= 12
        else:
            within("host refine value %d" % j, lt[2 + j], want["values"][j].val, want["values"][j].bound)
    assert [float(x) for x in ra[6]] == want["counts"]
    if want["num"] > 0:
        idx = want["idx"]
        tg = want["rows_out"]["pos"].astype(np.int64)[idx]
        ce_tol, tol_d = ce_mean_tolerance(cls[idx], tg, dict(ce_rows=want["ce_rows"], dcls_rows=want["dcls"][idx].copy()))
        within("host refine ce", lt[1], want["ce"], ce_tol)
        total = want["reg_loss"].val + want["ce"]
        within("host refine loss", lt[0], total, want["reg_loss"].bound + ce_tol + ref.U * abs(total))
        within("host refine dreg", host(gra), want["dreg"], want["dreg_bound"])
        got_dcls = host(gca)
        assert (got_dcls[~want["drawn"]] == 0).all()
        within("host refine dcls", got_dcls[idx], want["dcls"][idx], tol_d)
    else:
        assert lt[0] == 0 and lt[1] == 0 and branch in ("no_positive", "no_negative")


# ---- rejected shapes -------------------------------------------------------------------------------------------------------------
def test_rejected_and_empty_shapes(L):
    cls, reg, centre, tmpl, label = ref.stage2_case(4, 4, 900, labelled=1.0)
    t = [dev(x) for x in (cls, reg, centre, tmpl, label)]
    w = (ctypes.c_float * 4)(1, 1, 1, 1)
    o = dict(ng=full((4, 10)), pick=full((4,), torch.int32, -7), g8=full((4,), torch.int32, -7), ag=full((4, 7)), terms=full((4, 20)),
             dreg=full((4, 4, 10)), flags=full((12,), torch.uint8, 9), wide=full((4,), torch.int32, -7))

    def stage2(A=4, C=10, centre_ld=3, label_ld=10, m=4):
        return L.regnet_stage2_loss_rows_f32(t[0].data_ptr(), t[1].data_ptr(), A, C, t[2].data_ptr(), centre_ld, t[3].data_ptr(),
                                             t[4].data_ptr(), label_ld, RADIUS, ctypes.addressof(w), None, m, o["ng"].data_ptr(),
                                             o["pick"].data_ptr(), o["g8"].data_ptr(), o["ag"].data_ptr(), o["terms"].data_ptr(),
                                             o["dreg"].data_ptr(), stream())

    def refine(C=10, grasp_ld=10, label_ld=10, m=4):
        return L.regnet_refine_loss_rows_f32(t[4].data_ptr(), grasp_ld, t[0].data_ptr(), t[4].data_ptr(), t[4].data_ptr(), label_ld,
                                             C, RADIUS, THRE, m, o["ng"].data_ptr(), o["flags"].data_ptr(), o["terms"].data_ptr(),
                                             o["dreg"].data_ptr(), stream())

    assert stage2(C=9) == ERR_SHAPE and stage2(C=11) == ERR_SHAPE and stage2(label_ld=9) == ERR_SHAPE
    assert stage2(centre_ld=2) == ERR_SHAPE and stage2(A=0) == ERR_SHAPE and stage2(m=-1) == ERR_SHAPE
    assert stage2(A=65) == ERR_UNSUPPORTED
    assert refine(C=9) == ERR_SHAPE and refine(grasp_ld=9) == ERR_SHAPE and refine(label_ld=9) == ERR_SHAPE
    assert stage2(m=0) == OK and refine(m=0) == OK
    idx, tg = dev(np.zeros(1, dtype=np.int64)), dev(np.zeros(1, dtype=np.int32))
    assert L.regnet_ce_rows_f32(t[0].data_ptr(), 4, tg.data_ptr(), idx.data_ptr(), None, 0, 1.0, o["ng"].data_ptr(),
                                o["dreg"].data_ptr(), stream()) == OK
    assert L.regnet_ce_rows_f32(t[0].data_ptr(), 0, tg.data_ptr(), idx.data_ptr(), None, 1, 1.0, o["ng"].data_ptr(),
                                o["dreg"].data_ptr(), stream()) == ERR_SHAPE
    packed, gcount, centre6 = ref.label_case([3], 2, 901)
    p, g, c = dev(packed), dev(gcount), dev(centre6)
    for B, Nc in ((0, 2), (1, 0)):
        assert L.regnet_label_match_f32(p.data_ptr(), g.data_ptr(), packed.shape[1], c.data_ptr(), 12, 6, B, Nc, DEPTH, MAX_SQ,
                                        o["ng"].data_ptr(), o["wide"].data_ptr(), stream()) == OK
    assert L.regnet_label_match_f32(p.data_ptr(), g.data_ptr(), packed.shape[1], c.data_ptr(), 12, 6, -1, 2, DEPTH, MAX_SQ,
                                    o["ng"].data_ptr(), o["wide"].data_ptr(), stream()) == ERR_SHAPE
    for key, value in o.items():                                     # nothing was launched: every output keeps its fill
        fill = 9 if key == "flags" else -7 if value.dtype == torch.int32 else np.float32(SENT)
        assert (host(value) == fill).all(), key
