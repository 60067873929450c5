"""Pose non-maximum suppression + top-K restated in numpy float32, from the contract alone (DESIGN.md par. 5, "pose NMS"):
individually rounded binary32 operations in the written order.  numpy rounds every float32 operation on its own (there is no
contraction), for scalars and element-wise over arrays alike.

Inputs per grasp: centre c (3), frame columns a (approach), b (axis_y), m (minor normal) -- ``frame[i]`` is (3,3) with those as
COLUMNS, what ``eval_collision.grasp_frames`` returns -- and a score.

  close     d2 = ((dx dx) + (dy dy)) + (dz dz) <= T2,  T2 = float32(t) * float32(t)          (inclusive)
  aligned   tr = (da + db) + dm >= C,  da = ((ax ax') + (ay ay')) + (az az'), likewise db, dm;
            C = float32(1 + 2 cos(theta)) with the right-hand side evaluated in float64
            symmetric: tr2 = (da - db) - dm, max(tr, tr2) >= C
  same      close and aligned
  rank      descending score, NaN as -inf, equal scores by lower index
  greedy    walk the ranks; keep one unless an already kept one is the same grasp; stop at top_k kept (None / <= 0: no limit)
  output    keep (n) int64: kept input indices in rank order, then -1;  count

``pose_nms_plain`` is the plain double loop over scalars.  ``pose_nms_ref`` is the same double loop with the inner one -- over
the grasps kept so far -- carried out element-wise on float32 arrays, so that 16 000 grasps take seconds; the CPU tests hold the
two against one another.
"""
import math

import numpy as np

f32 = np.float32


def thresholds(translation_thresh, rotation_thresh_deg):
    t = f32(translation_thresh)
    return f32(t * t), f32(1.0 + 2.0 * math.cos(math.radians(float(rotation_thresh_deg))))


def rank_order(score):
    s = np.array(score, dtype=np.float32).reshape(-1)
    s[np.isnan(s)] = -np.inf
    return np.argsort(-s, kind="stable").astype(np.int64)      # (-0.0 == 0.0: a tie, broken by index)


def _dot(u, v):
    """((u0 v0) + (u1 v1)) + (u2 v2), float32 scalars or arrays (..., 3)."""
    return (u[..., 0] * v[..., 0] + u[..., 1] * v[..., 1]) + u[..., 2] * v[..., 2]


def same_grasp(c1, F1, c2, F2, T2, C, symmetric):
    """One pair.  c (3,), F (3,3) float32; F2 / c2 may carry leading dimensions (one grasp against many)."""
    c1, F1, c2, F2 = (np.asarray(x, dtype=np.float32) for x in (c1, F1, c2, F2))
    d = c1 - c2
    d2 = _dot(d, d)
    da = _dot(F1[..., :, 0], F2[..., :, 0])
    db = _dot(F1[..., :, 1], F2[..., :, 1])
    dm = _dot(F1[..., :, 2], F2[..., :, 2])
    tr = (da + db) + dm
    if symmetric:
        tr = np.maximum(tr, (da - db) - dm)
    with np.errstate(invalid="ignore"):
        return (d2 <= T2) & (tr >= C)


def _finish(kept, n):
    keep = np.full((n,), -1, dtype=np.int64)
    keep[:len(kept)] = kept
    return keep, len(kept)


def pose_nms_plain(center, frame, score, translation_thresh=0.03, rotation_thresh_deg=30.0, top_k=None, symmetric=True):
    """The contract as a plain double loop over scalars -> (keep, count)."""
    center, frame = np.asarray(center, dtype=np.float32), np.asarray(frame, dtype=np.float32)
    n = len(center)
    T2, C = thresholds(translation_thresh, rotation_thresh_deg)
    limit = n if top_k is None or top_k <= 0 else top_k
    kept = []
    for i in rank_order(score):
        if len(kept) >= limit:
            break
        for j in kept:
            if bool(same_grasp(center[i], frame[i], center[j], frame[j], T2, C, symmetric)):
                break
        else:
            kept.append(int(i))
    return _finish(kept, n)


def pose_nms_ref(center, frame, score, translation_thresh=0.03, rotation_thresh_deg=30.0, top_k=None, symmetric=True):
    """The same walk; each rank is compared with all kept grasps at once -> (keep, count)."""
    center, frame = np.asarray(center, dtype=np.float32), np.asarray(frame, dtype=np.float32)
    n = len(center)
    T2, C = thresholds(translation_thresh, rotation_thresh_deg)
    limit = n if top_k is None or top_k <= 0 else top_k
    kept = []
    kc, kF = np.empty((n, 3), dtype=np.float32), np.empty((n, 3, 3), dtype=np.float32)
    for i in rank_order(score):
        k = len(kept)
        if k >= limit:
            break
        if k and same_grasp(center[i], frame[i], kc[:k], kF[:k], T2, C, symmetric).any():
            continue
        kc[k], kF[k] = center[i], frame[i]
        kept.append(int(i))
    return _finish(kept, n)


def same_matrix(center, frame, rows, cols, translation_thresh, rotation_thresh_deg, symmetric):
    """bool (len(rows), len(cols)): is grasp rows[r] the same grasp as grasp cols[c]."""
    center, frame = np.asarray(center, dtype=np.float32), np.asarray(frame, dtype=np.float32)
    T2, C = thresholds(translation_thresh, rotation_thresh_deg)
    out = np.empty((len(rows), len(cols)), dtype=bool)
    for r, i in enumerate(rows):
        out[r] = same_grasp(center[i], frame[i], center[cols], frame[cols], T2, C, symmetric)
    return out


# ---- test inputs ----------------------------------------------------------------------------------------------------------
def rotation(axis, angle):
    """Rodrigues' formula in float64."""
    axis = np.asarray(axis, dtype=np.float64)
    axis = axis / np.linalg.norm(axis)
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + math.sin(angle) * K + (1 - math.cos(angle)) * (K @ K)


def random_frames(rng, n):
    """n right-handed orthonormal frames (float64) from QR."""
    q, _ = np.linalg.qr(rng.standard_normal((n, 3, 3)))
    q[:, :, 2] *= np.sign(np.linalg.det(q))[:, None]
    return q


def clustered_poses(seed, n, clusters=None, spread=0.004, wobble_deg=8.0, flip=0.3, extent=0.3):
    """Clustered grasps: ``clusters`` random centres / frames, every member its cluster's pose with a jittered centre, a small
    extra rotation and, with probability ``flip``, a half turn about the approach axis.  -> centre (n,3), frame (n,3,3), score
    (n) float32."""
    rng = np.random.default_rng(seed)
    clusters = max(1, n // 6) if clusters is None else clusters
    cc = rng.uniform(-extent, extent, (clusters, 3))
    cF = random_frames(rng, clusters)
    member = rng.integers(0, clusters, n)
    center = cc[member] + rng.normal(0.0, spread, (n, 3))
    frame = np.empty((n, 3, 3))
    half_turn = np.diag([1.0, -1.0, -1.0])
    for i in range(n):
        R = rotation(rng.standard_normal(3), math.radians(wobble_deg) * rng.uniform(-1, 1))
        frame[i] = R @ cF[member[i]]
        if rng.uniform() < flip:
            frame[i] = frame[i] @ half_turn
    score = rng.uniform(0.0, 1.0, n)
    return center.astype(np.float32), frame.astype(np.float32), score.astype(np.float32)


def grasps_from_poses(center, frame, score):
    """(n,8) float32 rows [centre, axis_y, angle, score] whose ``eval_collision.grasp_frames`` are close to ``frame`` (the
    tests read the frames back from grasp_frames; this only has to produce varied, clustered rows)."""
    center, frame = np.asarray(center, dtype=np.float64), np.asarray(frame, dtype=np.float64)
    b = frame[:, :, 1]
    x = np.stack([b[:, 1], -b[:, 0], np.zeros(len(b))], axis=1)
    x /= np.maximum(np.linalg.norm(x, axis=1, keepdims=True), 1e-12)
    z = np.cross(x, b)
    a = frame[:, :, 0]
    angle = np.arctan2((a * z).sum(1), (a * x).sum(1))        # grasp_frames: approach = cos(angle) x + sin(angle) z
    out = np.zeros((len(center), 8), dtype=np.float32)
    out[:, :3], out[:, 3:6], out[:, 6], out[:, 7] = center, b, angle, score
    return out


# ---- hand-derived known answers --------------------------------------------------------------------------------------------
T_EXACT = 0.03125            # 2^-5: float32(t) and T2 = 2^-10 are exact


def trace(F1, F2, symmetric=False):
    """tr (or max(tr, tr2)) of two float32 frames in the contract's arithmetic."""
    F1, F2 = np.asarray(F1, dtype=np.float32), np.asarray(F2, dtype=np.float32)
    da, db, dm = (_dot(F1[:, k], F2[:, k]) for k in range(3))
    tr = (da + db) + dm
    return max(tr, (da - db) - dm) if symmetric else tr


def known_cases():
    """-> list of (name, center, frame, score, kwargs, expected kept indices).  Every expectation is derived by hand from the
    contract; the asserts below pin the premises the derivations rest on."""
    I = np.eye(3, dtype=np.float32)
    zero = np.zeros(3, dtype=np.float32)
    cases = []

    def add(name, centers, frames, scores, expected, **kw):
        cases.append((name, np.asarray(centers, dtype=np.float32).reshape(-1, 3),
                      np.asarray(frames, dtype=np.float32).reshape(-1, 3, 3), np.asarray(scores, dtype=np.float32), kw, expected))

    # two identical poses: the higher score survives
    add("identical", [zero, zero], [I, I], [0.2, 0.9], [1])
    # centres exactly t apart on one axis: d2 = t * t = T2, the bound is inclusive; one float further: kept
    t = f32(T_EXACT)
    assert float(t) == T_EXACT and float(t * t) == T_EXACT ** 2
    above = np.nextafter(t, f32(1.0))
    assert above > t and f32(above * above) > f32(t * t)
    for axis in range(3):
        at, over = zero.copy(), zero.copy()
        at[axis], over[axis] = t, above
        add("exactly_t_axis%d" % axis, [zero, at], [I, I], [0.9, 0.5], [0], translation_thresh=T_EXACT)
        add("just_over_t_axis%d" % axis, [zero, over], [I, I], [0.9, 0.5], [0, 1], translation_thresh=T_EXACT)
    # b and m negated (half a turn about the approach axis): tr = 1 - 1 - 1 = -1, tr2 = 1 + 1 + 1 = 3
    flipped = I * np.array([1, -1, -1], dtype=np.float32)
    add("half_turn_symmetric", [zero, zero], [I, flipped], [0.9, 0.5], [0], symmetric=True)
    add("half_turn_asymmetric", [zero, zero], [I, flipped], [0.9, 0.5], [0, 1], symmetric=False)
    # a frame turned about its approach axis by a hair less / more than theta
    theta = 30.0
    _, C = thresholds(0.03, theta)
    base = rotation([0.3, -0.5, 0.8], 0.7)                                       # some frame, float64
    hair = 1e-4                                                                    # rad: 2 sin(theta) * hair = 1e-4 >> 2^-22
    for name, angle, expected in (("rotation_hair_less", math.radians(theta) - hair, [0]),
                                  ("rotation_hair_more", math.radians(theta) + hair, [0, 1])):
        turned = rotation(base[:, 0], angle) @ base
        F1, F2 = base.astype(np.float32), turned.astype(np.float32)
        for sym in (False, True):
            side = trace(F1, F2, sym) >= C
            assert side == (len(expected) == 1), (name, sym, trace(F1, F2, sym), C)   # the rounded frames land on the intended side
            add("%s_sym%d" % (name, sym), [zero, zero], [F1, F2], [0.9, 0.5], expected, rotation_thresh_deg=theta, symmetric=sym)
    # equal scores: index order (three distinct poses, far apart)
    far = np.array([[0, 0, 0], [1, 0, 0], [2, 0, 0]], dtype=np.float32)
    add("equal_scores", far, [I, I, I], [0.5, 0.5, 0.5], [0, 1, 2])
    add("signed_zero_scores", far, [I, I, I], [-0.0, 0.0, -0.0], [0, 1, 2])
    # NaN ranks last (as -inf: behind a real -inf only by index)
    add("nan_last", far, [I, I, I], [np.nan, 0.1, 0.7], [2, 1, 0])
    add("nan_and_minus_inf", far, [I, I, I], [np.nan, -np.inf, 0.7], [2, 0, 1])
    # top_k truncates the greedy list
    add("top_k", far, [I, I, I], [0.1, 0.9, 0.5], [1, 2], top_k=2)
    add("top_k_zero_is_no_limit", far, [I, I, I], [0.1, 0.9, 0.5], [1, 2, 0], top_k=0)
    # suppression is by KEPT grasps only: 1 is the same as 0 and is dropped, so 2 (the same as 1, not as 0) survives
    chain = np.array([[0, 0, 0], [0.02, 0, 0], [0.04, 0, 0]], dtype=np.float32)
    add("chain", chain, [I, I, I], [0.9, 0.8, 0.7], [0, 2], translation_thresh=T_EXACT)
    return cases
