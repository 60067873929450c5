"""Approach analysis on the MI355X (csrc/approach.hip through approach.py) against the numpy restatement of the contract
(tests/approach_reference.py).  Every comparison is exact, counts and values: the contract is fp32 multiply, add, compare, min and
max in a fixed order, and integer counts.  The reference is fed the global->local matrices the device computed
(eval_collision.grasp_frames / global_to_local, downloaded): the kernel takes matrices, so no sin / cos sits inside what is
compared."""
import functools

import numpy as np
import pytest
import torch

from . import approach_reference as ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
f32 = np.float32
WIDTH, DEPTH = 0.08, 0.06
GRIPPER = ref.gripper_box(DEPTH, WIDTH)                     # x_lo -0.06, x_hi 0.06, ht 0.005, hw 0.05, hs 0.04, back_x -0.0
STANDOFF, CONTACT_DEPTH, FRICTION = 0.1, ref.NEIGHBOR_DEPTH, 30.0
IDENTITY = np.eye(4, dtype=np.float32)[None]
SENTINEL = -77


def _dev(a, dtype=np.float32):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(DEV)


def _kernel(points, normals, T, box, standoff, contact_depth, cos_fric, counts=None, values=None):
    """The C entry point on device tensors (any strides for points / normals) -> (counts, values) as numpy arrays."""
    from regnet_for_3d_grasping_amd import _lib
    B, N = int(T.shape[0]), int(points.shape[0])
    x_lo, x_hi, ht, hw, hs, back_x = box
    per = _dev(x_hi) if np.ndim(x_hi) else None
    if counts is None:
        counts = torch.full((B, 8), SENTINEL, dtype=torch.int32, device=DEV)
        values = torch.full((B, 4), float(SENTINEL), dtype=torch.float32, device=DEV)
    n_args = (None, 0, 0) if normals is None else (normals.data_ptr(), normals.stride(0), normals.stride(1))
    _lib.call("regnet_grasp_approach_f32", points, points.data_ptr(), points.stride(0), points.stride(1), *n_args, N,
              T.data_ptr(), B, float(x_lo), 0.0 if per is not None else float(x_hi), None if per is None else per.data_ptr(),
              float(ht), float(hw), float(hs), float(back_x), float(standoff), float(contact_depth), float(cos_fric),
              counts.data_ptr(), values.data_ptr())
    return counts.cpu().numpy(), values.cpu().numpy()


def _same(got, want, what=""):
    assert got[0].dtype == np.int32 and got[1].dtype == np.float32
    assert np.array_equal(got[0], want[0]), (what, got[0], want[0])
    assert got[1].tobytes() == want[1].tobytes(), (what, got[1], want[1])


def _run_identity(points, normals, box=GRIPPER, standoff=STANDOFF, contact_depth=CONTACT_DEPTH, cos_fric=None):
    """One grasp with the identity matrix, so that the local coordinates are the inputs exactly -> (counts[0], values[0]),
    already held against the restatement."""
    cf = ref.cos_friction(FRICTION) if cos_fric is None else cos_fric
    points = np.asarray(points, dtype=np.float32).reshape(-1, 3)
    normals = None if normals is None else np.asarray(normals, dtype=np.float32).reshape(-1, 3)
    got = _kernel(_dev(points), _dev(normals), _dev(IDENTITY), box, standoff, contact_depth, cf)
    _same(got, ref.approach_ref(points, normals, IDENTITY, box, standoff, contact_depth, cf))
    return got[0][0], got[1][0]


# ---- random clouds around the hands, through analyse ----------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _case(N, B):
    grasp, points, normals = ref.random_case(1000 * B + N, N, B)
    return _dev(grasp), _dev(points), _dev(normals)


def _analyse_and_check(points, grasp, depth, normals, friction=FRICTION, **kw):
    from regnet_for_3d_grasping_amd import approach, eval_collision
    params = approach.ApproachParams(friction_deg=friction, **kw)
    res = approach.analyse(points, grasp, depth, WIDTH, params, normals=normals)
    B = grasp.shape[0]
    assert res.counts.shape == (B, 8) and res.counts.dtype == torch.int32 and res.counts.device == points.device
    assert res.values.shape == (B, 4) and res.values.dtype == torch.float32
    T = eval_collision.global_to_local(res.frame, res.center).cpu().numpy()
    host_depth = depth.cpu().numpy() if isinstance(depth, torch.Tensor) else depth
    box = ref.gripper_box(host_depth, WIDTH)
    want = ref.approach_ref(points.cpu().numpy(), None if (normals is None or friction is None) else normals.cpu().numpy(), T, box,
                            params.standoff, params.contact_depth, 0.0 if friction is None else ref.cos_friction(friction))
    _same((res.counts.cpu().numpy(), res.values.cpu().numpy()), want)
    derived = ref.derived_ref(want[0], want[1], res.frame.cpu().numpy(), res.center.cpu().numpy(), params.pad, box[4])
    got = dict(zip(derived, (res.clearance, res.width, res.offset, res.opening, res.contact, res.pregrasp)))
    for key, value in derived.items():
        assert got[key].dtype == torch.float32 and got[key].cpu().numpy().tobytes() == value.tobytes(), key
    return res, want


@pytest.mark.parametrize("B", [0, 1, 3])
@pytest.mark.parametrize("N", [0, 1, 63, 64, 255, 256, 257, 1000])
def test_random_clouds_around_the_hand(N, B):
    grasp, points, normals = _case(N, B)
    per_grasp = _dev(np.random.default_rng(N + B).uniform(0.03, 0.08, B))
    for depth in (DEPTH, per_grasp):
        _, want = _analyse_and_check(points, grasp, depth, normals)
    # the same cloud as a transposed (3,N).T view: strides (1, N)
    view_p, view_n = points.t().contiguous().t(), normals.t().contiguous().t()
    assert N < 2 or (not view_p.is_contiguous() and view_p.stride() == (1, N))
    _, again = _analyse_and_check(view_p, grasp, per_grasp, view_n)
    _same(again, want)
    if N == 1000 and B == 3:                             # not vacuous: a partly free approach, both bands, both verdicts
        counts, values = want
        assert (counts[:, 0] > 0).all() and (counts[:, 1] > 0).any() and (counts[:, 3] > counts[:, 4]).any() and (counts[:, 4] > 0).any()
        assert ((values[:, 2] > 0) & (values[:, 2] < f32(STANDOFF))).any()


def test_side_stream_and_two_runs_give_the_same_bytes():
    from regnet_for_3d_grasping_amd import approach
    grasp, points, normals = _case(1000, 3)
    params = approach.ApproachParams(friction_deg=FRICTION)
    _, want = _analyse_and_check(points, grasp, DEPTH, normals)
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        a = approach.analyse(points, grasp, DEPTH, WIDTH, params, normals=normals)
        b = approach.analyse(points, grasp, DEPTH, WIDTH, params, normals=normals)
    side.synchronize()
    assert a.counts.cpu().numpy().tobytes() == b.counts.cpu().numpy().tobytes() == want[0].tobytes()
    assert a.values.cpu().numpy().tobytes() == b.values.cpu().numpy().tobytes() == want[1].tobytes()


def test_estimated_normals_and_no_normals():
    from regnet_for_3d_grasping_amd import approach, eval_collision
    grasp, points, normals = _case(1000, 3)
    est = eval_collision.estimate_normals(points, radius=0.02, max_nn=20)
    res, _ = _analyse_and_check(points, grasp, DEPTH, est, normal_radius=0.02, normal_max_nn=20)
    own = approach.analyse(points, grasp, DEPTH, WIDTH, {"friction_deg": FRICTION, "normal_radius": 0.02, "normal_max_nn": 20})
    assert torch.equal(own.counts, res.counts) and torch.equal(own.values, res.values)      # it estimates them itself
    # friction_deg None: no pass 2 even when normals are handed in; normals=None with it: the same
    for given in (normals, None):
        off, want = _analyse_and_check(points, grasp, DEPTH, given, friction=None)
        assert not want[0][:, 3:].any() and not off.contact.any() and torch.equal(off.counts[:, :3], res.counts[:, :3])
        assert torch.equal(off.values, res.values)


# ---- known answers ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ref.known_cases(), ids=lambda c: c[0])
def test_known_answers_through_the_kernel(case):
    _, inputs, counts, values = case
    got = _kernel(_dev(inputs["points"]), _dev(inputs["normals"]), _dev(inputs["T"]), inputs["box"], inputs["standoff"],
                  inputs["contact_depth"], inputs["cos_friction"])
    _same(got, (counts, values))


# ---- every threshold at one ulp ---------------------------------------------------------------------------------------------------
def _three(v):
    """just below, at, just above a float32 (towards -inf / +inf)."""
    v = f32(v)
    return np.nextafter(v, f32(-np.inf)), v, np.nextafter(v, f32(np.inf))


X_LO, X_HI, HT, HW, HS, _ = GRIPPER
ULP_BOX = (X_LO, X_HI, HT, HW, HS, f32(-0.0125))           # a palm face off zero, so that its neighbours are normal numbers
N_REGION, N_BLOCK, N_HAND = 0, 1, 2


def _planted(make_point, at, pick, expected, box=GRIPPER):
    """``make_point(v)`` -> one point for each of just below / at / just above ``at``; ``pick(counts, values)`` of the three runs
    must be ``expected`` (and every run equals the restatement)."""
    seen = [pick(*_run_identity([make_point(v)], None, box=box)) for v in _three(at)]
    assert seen == list(expected), (seen, expected)


def test_sweep_thresholds_at_one_ulp():
    S = f32(STANDOFF)
    blocks = lambda c, v: int(c[N_BLOCK])
    # the far end of the sweep, x_lo - S in float32: strict
    _planted(lambda v: (v, 0.0, 0.0), f32(X_LO - S), blocks, (0, 0, 1))
    _planted(lambda v: (v, 0.045, 0.0), f32(X_LO - S), blocks, (0, 0, 1))
    # x_lo: a blocker on either side; the clearance is 1 ulp below, 0 at and above; the region starts strictly above
    _planted(lambda v: (v, 0.0, 0.0), X_LO, lambda c, v: (int(c[N_BLOCK]), int(c[N_REGION]), float(v[2]) > 0),
             ((1, 0, True), (1, 0, False), (1, 1, False)))
    below = np.nextafter(X_LO, f32(-np.inf))
    _, values = _run_identity([(below, 0.0, 0.0)], None)
    assert values[2] == f32(X_LO - below) and 0 < values[2] < 1e-8
    # the palm face for an inner point (back_x), the finger tips for a finger-lane point (x_hi): strict
    _planted(lambda v: (v, 0.0, 0.0), ULP_BOX[5], blocks, (1, 0, 0), box=ULP_BOX)
    _planted(lambda v: (v, 0.0, 0.0), ULP_BOX[5], lambda c, v: int(c[N_HAND]), (1, 0, 0), box=ULP_BOX)
    for y in (0.045, -0.045):
        _planted(lambda v: (v, y, 0.0), X_HI, lambda c, v: (int(c[N_BLOCK]), int(c[N_HAND])), ((1, 1), (0, 0), (0, 0)))
    # the gripper's own palm face is -0.0: neither zero is behind it, the nearest normal numbers on either side are / are not
    seen = [int(_run_identity([(x, 0.0, 0.0)], None)[0][N_BLOCK]) for x in (-1e-30, -0.0, 0.0, 1e-30)]
    assert seen == [1, 0, 0, 0]


def test_section_thresholds_at_one_ulp():
    inside = lambda c, v: (int(c[N_REGION]), int(c[N_HAND]), int(c[N_BLOCK]))
    for sign in (1.0, -1.0):
        order = (lambda t: t) if sign > 0 else (lambda t: t[::-1])          # (mirrored: "below" is the inner side)
        # |y| = hs at x inside the fingers' reach: region inside, the lane itself is a blocker but neither region nor finger
        _planted(lambda v: (0.03, v, 0.0), sign * HS, inside, order(((1, 0, 0), (0, 0, 1), (0, 1, 1))))
        # |y| = hw: a finger inside, nothing at and beyond
        _planted(lambda v: (0.03, v, 0.0), sign * HW, inside, order(((0, 1, 1), (0, 0, 0), (0, 0, 0))))
        # |z| = ht, for a region point, a finger point and a blocker behind the palm
        _planted(lambda v: (0.03, 0.0, v), sign * HT, inside, order(((1, 0, 0), (0, 0, 0), (0, 0, 0))))
        _planted(lambda v: (0.03, 0.045, v), sign * HT, inside, order(((0, 1, 1), (0, 0, 0), (0, 0, 0))))
        _planted(lambda v: (-0.1, 0.0, v), sign * HT, inside, order(((0, 0, 1), (0, 0, 0), (0, 0, 0))))


def test_band_and_friction_thresholds_at_one_ulp():
    y_lo, y_hi, cd = f32(-0.03), f32(0.03), f32(CONTACT_DEPTH)
    assert f32(y_hi - y_lo) / f32(3.0) > cd                                 # the band is contact_depth
    left_edge, right_edge = f32(y_hi - cd), f32(y_lo + cd)
    ends = [(0.03, y_lo, 0.0), (0.03, y_hi, 0.0)]
    along = [(0.0, 1.0, 0.0)] * 3
    for edge, column, expected in ((left_edge, 3, (1, 1, 2)), (right_edge, 5, (2, 1, 1))):      # strictly inside the band
        seen = [int(_run_identity(ends + [(0.03, v, 0.0)], along)[0][column]) for v in _three(edge)]
        assert seen == list(expected), (column, seen)
    # a span under 3 contact depths: the band is the third, (y_max - y_min) / 3.0f
    y_hi2 = f32(-0.03 + 0.009)
    third = f32(f32(y_hi2 - y_lo) / f32(3.0))
    assert third < cd
    seen = [int(_run_identity([(0.03, y_lo, 0.0), (0.03, y_hi2, 0.0), (0.03, v, 0.0)], along)[0][3]) for v in _three(f32(y_hi2 - third))]
    assert seen == [1, 1, 2]
    # |n_y| against cos_friction: inclusive, either sign, on the left band's one point
    cf = ref.cos_friction(FRICTION)
    for sign in (1.0, -1.0):
        seen = []
        for c in _three(cf):
            counts, _ = _run_identity(ends, [(0.0, 1.0, 0.0), (0.6, sign * c, 0.0)])
            assert counts[3] == 1 and counts[5] == 1 and counts[6] == 1
            seen.append(int(counts[4]))
        assert seen == [0, 1, 1]


# ---- reductions: the deciding point in every wave and in the tail ----------------------------------------------------------------
@pytest.mark.parametrize("row", [0, 64, 128, 255, 256, -1])
def test_the_extreme_point_is_found_in_every_row(row):
    N = 300
    rng = np.random.default_rng(9)
    base = np.zeros((N, 3), dtype=np.float32)
    base[:, 0] = np.where(np.arange(N) % 2 == 0, rng.uniform(0.01, 0.05, N), rng.uniform(-0.15, -0.11, N))     # object | wall
    base[:, 1] = rng.uniform(-0.02, 0.02, N)
    normals = np.tile(np.array([[0.0, 1.0, 0.0]], dtype=np.float32), (N, 1))
    _, plain = _run_identity(base, normals)
    assert f32(0.05) <= plain[2] <= f32(0.09) and plain[0] >= f32(-0.02) and plain[1] <= f32(0.02)
    for point, column in (((-0.07, 0.0, 0.0), 2), ((0.03, -0.035, 0.0), 0), ((0.03, 0.035, 0.0), 1)):
        cloud = base.copy()
        cloud[row] = point
        _, values = _run_identity(cloud, normals)
        want = f32(X_LO - f32(point[0])) if column == 2 else f32(point[1])
        assert values[column] == want, (row, column, values)


# ---- degenerate inputs ------------------------------------------------------------------------------------------------------------
def test_degenerate_inputs():
    from regnet_for_3d_grasping_amd import approach
    # an empty region: the +-inf values, zero derived tensors, the whole standoff free
    far = np.array([[0.5, 0.5, 0.5], [0.03, 0.0, 0.2]], dtype=np.float32)
    counts, values = _run_identity(far, [(0, 1, 0)] * 2)
    assert not counts.any() and values.tolist() == [np.inf, -np.inf, f32(STANDOFF), np.inf]
    grasp = torch.zeros((1, 8), device=DEV)
    grasp[0, 4] = 1.0                                                       # at the origin, closing along y, approach along x
    res = approach.analyse(_dev(far), grasp, DEPTH, WIDTH, {"friction_deg": FRICTION}, normals=_dev([(0, 1, 0)] * 2))
    assert res.counts[0, 0].item() == 0 and res.values[0].tolist() == [np.inf, -np.inf, f32(STANDOFF), np.inf]
    for t in (res.width, res.offset, res.contact):
        assert t.tolist() == [0.0]
    assert res.opening.tolist() == [f32(f32(0.005) + f32(0.005))] and res.clearance.tolist() == [f32(STANDOFF)]
    assert res.pregrasp.cpu().numpy().tobytes() == np.array([[-f32(STANDOFF), 0.0, 0.0]], dtype=np.float32).tobytes()
    assert res.passes().tolist() == [True]
    # a one-point region: the band is 0 and both bands are empty
    counts, values = _run_identity([(0.03, 0.01, 0.0)], [(0, 1, 0)])
    assert counts.tolist() == [1, 0, 0, 0, 0, 0, 0, 0] and values.tolist() == [f32(0.01), f32(0.01), f32(STANDOFF), f32(0.03)]
    # NaN point rows are in nothing; NaN normals fail.  The cloud is drawn in the hand's own local coordinates.
    rng = np.random.default_rng(5)
    points_id = np.c_[rng.uniform(-0.2, 0.09, 600), rng.uniform(-0.06, 0.06, 600), rng.uniform(-0.008, 0.008, 600)].astype(np.float32)
    normals = np.c_[rng.normal(scale=0.4, size=600), np.ones(600), rng.normal(scale=0.4, size=600)]
    normals = (normals / np.linalg.norm(normals, axis=1, keepdims=True)).astype(np.float32)
    counts_all, _ = _run_identity(points_id, normals)
    holes = points_id.copy()
    holes[np.arange(0, 600, 3), rng.integers(0, 3, 200)] = np.nan            # one NaN coordinate in every third row
    counts_holes, values_holes = _run_identity(holes, normals)
    kept = np.arange(600) % 3 != 0
    counts_kept, values_kept = _run_identity(points_id[kept], normals[kept])
    assert np.array_equal(counts_holes, counts_kept) and values_holes.tobytes() == values_kept.tobytes()
    assert 0 < counts_holes[0] < counts_all[0]
    bad_normals = normals.copy()
    bad_normals[:, 1] = np.nan
    counts_nan, _ = _run_identity(points_id, bad_normals)
    assert counts_nan[3] == counts_all[3] > 0 and counts_nan[5] == counts_all[5] > 0 and counts_nan[4] == 0 and counts_nan[6] == 0
    assert 0 < counts_all[4] < counts_all[3] and 0 < counts_all[6]
    # S = 0: nothing behind the palm counts; a point inside the hand still does
    counts, values = _run_identity([(-0.07, 0.0, 0.0)], None, standoff=0.0)
    assert counts[N_BLOCK] == 0 and values[2] == 0.0 and np.signbit(values[2]) == False   # noqa: E712
    counts, values = _run_identity([(-0.03, 0.0, 0.0)], None, standoff=0.0)
    assert counts[N_BLOCK] == 1 and values[2] == 0.0
    # a point at exactly x == x_lo: clearance 0 (and +0.0), not part of the region
    counts, values = _run_identity([(X_LO, 0.0, 0.0)], None)
    assert counts[N_BLOCK] == 1 and counts[N_REGION] == 0 and values[2] == 0.0 and not np.signbit(values[2])
    # -0.0 never leaves the kernel
    _, values = _run_identity([(0.03, -0.0, 0.0)], None)
    assert values[0] == 0.0 and not np.signbit(values[0]) and not np.signbit(values[1])
    # normals=None: pass 2's counts are 0
    counts, _ = _run_identity(points_id, None)
    assert np.array_equal(counts[:3], counts_all[:3]) and not counts[3:].any()


# ---- the ABI's errors: before any launch ------------------------------------------------------------------------------------------
def test_every_error_code_leaves_the_outputs_alone():
    from regnet_for_3d_grasping_amd import _lib
    points, T = _dev(np.zeros((5, 3))), _dev(np.repeat(IDENTITY, 2, axis=0))
    counts = torch.full((2, 8), SENTINEL, dtype=torch.int32, device=DEV)
    values = torch.full((2, 4), float(SENTINEL), dtype=torch.float32, device=DEV)
    stream = torch.cuda.current_stream(DEV).cuda_stream

    def raw(N=5, B=2, standoff=0.1, p=points.data_ptr(), t=T.data_ptr(), c=counts.data_ptr(), v=values.data_ptr()):
        return _lib.lib.regnet_grasp_approach_f32(p, 3, 1, None, 0, 0, N, t, B, -0.06, 0.06, None, 0.005, 0.05, 0.04, -0.0, standoff,
                                                  0.005, 0.5, c, v, stream)

    assert raw(N=-1) == -1 and raw(B=-1) == -1
    assert raw(N=1 << 31) == -3 and raw(B=1 << 31) == -3
    assert raw(standoff=-1e-3) == -3 and raw(standoff=float("nan")) == -3 and raw(standoff=float("inf")) == -3
    assert raw(p=None) == -2 and raw(t=None) == -2 and raw(c=None) == -2 and raw(v=None) == -2
    assert raw(B=0) == 0                                                    # nothing to do: no launch
    torch.cuda.synchronize()
    assert (counts == SENTINEL).all() and (values == float(SENTINEL)).all()
    with pytest.raises(RuntimeError, match="regnet_grasp_approach_f32 failed"):
        _kernel(points, None, T, GRIPPER, -1.0, 0.005, 0.5)
    assert raw(N=0, p=None) == 0                                            # an empty cloud launches and writes the empty results
    torch.cuda.synchronize()
    assert counts.tolist() == [[0] * 8] * 2 and values.tolist() == [[np.inf, -np.inf, f32(0.1), np.inf]] * 2


# ---- no host read -----------------------------------------------------------------------------------------------------------------
def test_graph_capture_has_no_host_read():
    from regnet_for_3d_grasping_amd import approach
    params = approach.ApproachParams(friction_deg=FRICTION, min_clearance=0.05)
    inputs = [_case(1000, 3), tuple(t.flip(0).contiguous() for t in _case(1000, 3))]
    inputs[1] = (inputs[1][0], inputs[1][1] + 0.001, inputs[1][2])
    grasp, points, normals = (t.clone() for t in inputs[0])
    depth = torch.full((3,), DEPTH, device=DEV)

    def run():
        res = approach.analyse(points, grasp, depth, WIDTH, params, normals=normals)
        return res, (res.counts, res.values, res.clearance, res.width, res.offset, res.opening, res.contact, res.pregrasp, res.passes())

    warm = torch.cuda.Stream(device=DEV)
    warm.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(warm):
        run()
    torch.cuda.current_stream(DEV).wait_stream(warm)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        res, outputs = run()
    for g, p, n in (inputs[0], inputs[1], inputs[0]):
        for t in outputs[:2]:
            t.fill_(SENTINEL)
        grasp.copy_(g)
        points.copy_(p)
        normals.copy_(n)
        graph.replay()
        torch.cuda.synchronize()
        eager, _ = run()
        assert eager.counts.cpu().numpy().tobytes() == outputs[0].cpu().numpy().tobytes()
        assert eager.values.cpu().numpy().tobytes() == outputs[1].cpu().numpy().tobytes()
        assert torch.equal(eager.pregrasp, outputs[7]) and torch.equal(eager.passes(), outputs[8])
        _analyse_and_check(p, g, depth, n)
