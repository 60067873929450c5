"""csrc/icp.hip's projective step against tests/icp_projective_reference.py on the device: every correspondence exactly -- the
pixel a point falls on at and around a half, the image's edges, the window at corners and borders, ties, the distance and
normal gates at their thresholds, missing pixels and normals --, the 29 sums within the rounding of a float64 sum of their
length, the loop on the rendered corner, what a finished registration no longer touches, the grid search's bytes through the
shared tail, and every new error code."""
import math

import numpy as np
import pytest
import torch

from . import icp_projective_reference as pref
from . import icp_reference as ref
from .test_icp_projective_reference_cpu import (CORNER_H, CORNER_K, CORNER_STEP, CORNER_W, DYADIC_K, corner_floor, corner_views,
                                                pixel_grid)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U = 2.0 ** -53
f32 = np.float32


def gpu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def one_step(source, target, normals, W, H, K, pose, max_dist, stride=1, window=1, source_normals=None, min_cos=None, min_pairs=0,
             state=None):
    """One projective step through the C entry point -> (idx, sums, state bytes), the sentinel -9 / NaN where nothing was written."""
    from regnet_for_3d_grasping_amd import _lib, registration
    source = np.asarray(source, dtype=np.float32).reshape(-1, 3)
    n = len(source)
    rows = -(-n // stride)
    src, tgt, nrm = gpu(source), gpu(np.asarray(target, dtype=np.float32)), gpu(np.asarray(normals, dtype=np.float32))
    sn = None if source_normals is None else gpu(np.asarray(source_normals, dtype=np.float32))
    if state is None:
        state = gpu(registration.initial_state(pose, {"iterations": 30}))
    idx = torch.full((max(rows, 1),), -9, dtype=torch.int32, device=DEV)
    sums = torch.full((29,), float("nan"), dtype=torch.float64, device=DEV)
    ws = torch.empty((registration.projective_workspace_bytes(n),), dtype=torch.uint8, device=DEV)
    k = np.array(K, dtype=np.float64)
    _lib.call("regnet_icp_step_projective_f32", src, src.data_ptr(), n, stride, None if sn is None else sn.data_ptr(), tgt.data_ptr(),
              nrm.data_ptr(), W, H, k.ctypes.data, window, state.data_ptr(), float(max_dist), -2.0 if min_cos is None else float(min_cos),
              idx.data_ptr(), sums.data_ptr(), min_pairs, ws.data_ptr())
    torch.cuda.synchronize()
    return idx[:rows].cpu().numpy(), sums.cpu().numpy(), state.cpu().numpy()


def unit_normals(rng, n):
    v = rng.normal(size=(n, 3))
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)


def scattered(rng, n, W, H, K):
    """n source rows on the half-pixel lattice of the image at depths k / 8 around 1 -- exact in float32, so pixels at a half and
    equal distances exist --, a margin of pixels beyond every edge, and a few rows behind the camera, at z = 0, NaN and Inf."""
    u = rng.randint(-4, 2 * W + 4, size=n) / 2.0
    v = rng.randint(-4, 2 * H + 4, size=n) / 2.0
    z = rng.randint(6, 11, size=n) / 8.0
    pts = np.stack([(u - K[2]) / K[0] * z, (v - K[3]) / K[1] * z, z], axis=1).astype(np.float32)
    if n:
        kind = rng.randint(0, 12, size=n)
        pts[kind == 0, 2] = 0.0
        pts[kind == 1, 2] *= -1
        pts[kind == 2, 0] = np.nan
        pts[kind == 3, 1] = np.inf
    return pts


def image_target(rng, W, H, K):
    """The pixel grid at z = 1 pushed to depths k / 8, a tenth of the pixels removed, a tenth without a normal."""
    xyz, _ = pixel_grid(W, H, K)
    xyz = xyz * (rng.randint(7, 10, size=(W * H, 1)) / 8.0).astype(np.float32)
    normals = unit_normals(rng, W * H)
    xyz[rng.rand(W * H) < 0.1] = np.nan
    normals[rng.rand(W * H) < 0.1, rng.randint(0, 3)] = np.nan
    return xyz, normals


@pytest.mark.parametrize("shape", [(1, 1), (3, 3), (64, 4), (67, 5)])
@pytest.mark.parametrize("n_s", [0, 1, 63, 64, 65, 257])
def test_correspondences_are_the_restatements(n_s, shape):
    W, H = shape
    rng = np.random.RandomState(1000 * n_s + 10 * W + H)
    K = (64.0, 64.0, (W - 1) / 2.0, (H - 1) / 2.0)
    target, normals = image_target(rng, W, H, K)
    source = scattered(rng, n_s, W, H, K)
    source_normals = unit_normals(rng, n_s)
    source_normals[rng.rand(n_s) < 0.1] = np.nan
    matched = 0
    for window, min_cos in ((0, None), (1, None), (2, None), (1, 0.0), (2, -1.0)):
        idx, sums, _ = one_step(source, target, normals, W, H, K, np.eye(4), 0.25, window=window, source_normals=source_normals,
                                min_cos=min_cos)
        want, _ = pref.correspond_projective(source, target, normals, W, H, K, np.eye(4), 0.25, window=window,
                                             source_normals=source_normals, min_cos=min_cos)
        assert idx.tolist() == want.tolist(), (window, min_cos)
        assert sums[28] == float((want >= 0).sum())
        matched += int((want >= 0).sum())
    if n_s >= 63 and W > 1:
        assert matched >= 20 and (want == -1).any() and (want == -2).any()       # (the cases are not empty)


def test_the_pixel_at_a_half_the_four_edges_and_points_the_camera_cannot_see():
    target, normals = pixel_grid(3, 3)
    half = f32(0.5) / f32(64)
    below = np.nextafter(half, f32(0))
    edge = f32(1.5 / 64)
    source = np.array([[half, 0, 1], [below, 0, 1], [np.nextafter(half, f32(1)), 0, 1], [-half, 0, 1], [-below, 0, 1],
                       [-edge, 0, 1], [np.nextafter(-edge, f32(-1)), 0, 1], [edge, 0, 1], [np.nextafter(edge, f32(0)), 0, 1],
                       [0, -edge, 1], [0, np.nextafter(-edge, f32(-1)), 1], [0, edge, 1], [0, np.nextafter(edge, f32(0)), 1],
                       [0, 0, 0], [0, 0, -1], [1 / 64, 1 / 64, -1], [np.nan, 0, 1], [0, 0, np.inf], [0, -np.inf, 1], [0, 0, np.nan]],
                      dtype=np.float32)
    for K in (DYADIC_K, (64.0, 64.0, 0.0, 0.0)):          # (without a principal point uf + 0.5 = 1 and an ulp below are told apart)
        for window in (0, 2):
            idx, _, _ = one_step(source, target, normals, 3, 3, K, np.eye(4), 1.0, window=window)
            want, _ = pref.correspond_projective(source, target, normals, 3, 3, K, np.eye(4), 1.0, window=window)
            assert idx.tolist() == want.tolist(), (K, window)
    idx, _, _ = one_step(source, target, normals, 3, 3, DYADIC_K, np.eye(4), 1.0, window=0)
    assert idx[[0, 2, 3, 5, 6, 7]].tolist() == [5, 5, 4, 3, -1, -1] and idx[9:12].tolist() == [1, -1, -1]     # a half rounds up
    assert idx[13:].tolist() == [-1, -1, -1, -2, -2, -2, -2]
    # without a principal point the sums stay below 2, where an ulp of the coordinate survives uf + 0.5: 2 exactly is pixel 2, an
    # ulp below pixel 1
    idx, _, _ = one_step(source, target, normals, 3, 3, (64.0, 64.0, 0.0, 0.0), np.eye(4), 1.0, window=0)
    assert idx[[0, 7, 8, 11, 12]].tolist() == [1, 2, 1, 6, 3] and idx[[5, 9]].tolist() == [-1, -1]


@pytest.mark.parametrize("window", [0, 1, 2])
def test_the_window_at_corners_and_borders(window):
    """Every pixel of a 5 x 4 image as a source point a little off its own surface point, the nearest target pixel moved away: the
    match is then decided among the window's other pixels, fewer of them at a corner or a border."""
    W, H = 5, 4
    K = (64.0, 64.0, 2.0, 1.5)
    target, normals = pixel_grid(W, H, K)
    source = target.copy()
    far = target.copy()
    far[:, 2] += f32(0.125)                                 # every pixel's own partner is 1/8 behind it ...
    far[::3, 2] -= f32(0.0625)                              # ... every third only 1/16
    idx, _, _ = one_step(source, far, normals, W, H, K, np.eye(4), 0.25, window=window)
    want, _ = pref.correspond_projective(source, far, normals, W, H, K, np.eye(4), 0.25, window=window)
    assert idx.tolist() == want.tolist()
    if window == 0:
        assert idx.tolist() == list(range(W * H))
    else:
        assert (idx != np.arange(W * H)).sum() >= 6 and idx[0] == 0 and (idx >= 0).all()


def test_ties_the_distance_and_normal_gates_missing_pixels_and_normals():
    target, normals = pixel_grid(3, 3)
    centre = np.array([[0, 0, 1]], dtype=np.float32)
    far = target.copy()
    far[:, 2] = 1.125
    far[[2, 6]] = [[1 / 64, 0, 1], [-1 / 64, 0, 1]]
    assert one_step(centre, far, normals, 3, 3, DYADIC_K, np.eye(4), 0.25)[0].tolist() == [2]              # equal d2: the lower row
    assert one_step(centre, far, normals, 3, 3, DYADIC_K, np.eye(4), 0.25, window=0)[0].tolist() == [4]
    far[[1, 3, 5, 7]] = [[0, 1 / 64, 1], [0, -1 / 64, 1], [1 / 64, 0, 1], [0, 0, 1 + 1 / 64]]              # six at 1/64: still the lowest
    assert one_step(centre, far, normals, 3, 3, DYADIC_K, np.eye(4), 0.25, window=2)[0].tolist() == [1]
    back = np.array([[0, 0, 1.25], [0, 0, np.nextafter(f32(1.25), f32(0))], [0, 0, np.nextafter(f32(1.25), f32(2))]], dtype=np.float32)
    idx, sums, _ = one_step(back, target, normals, 3, 3, DYADIC_K, np.eye(4), 0.25, window=0)
    assert idx.tolist() == [4, 4, -1] and sums[28] == 2.0                                                     # d2 at max2, below, above
    holed, no_normal = target.copy(), normals.copy()
    holed[4] = np.nan
    no_normal[3, 1] = np.nan
    assert one_step(centre, holed, no_normal, 3, 3, DYADIC_K, np.eye(4), 0.25)[0].tolist() == [1]
    assert one_step(centre, holed, normals, 3, 3, DYADIC_K, np.eye(4), 0.25, window=0)[0].tolist() == [-1]
    no_normal[:] = np.nan
    assert one_step(centre, target, no_normal, 3, 3, DYADIC_K, np.eye(4), 0.25, window=2)[0].tolist() == [-1]
    # the normal gate: the dot product is -s_z against (0, 0, -1); at min_cos, an ulp below (refused) and above
    c = f32(0.5)
    tilted = np.array([[0, np.sqrt(1 - float(v) ** 2), -v] for v in (c, np.nextafter(c, f32(0)), np.nextafter(c, f32(1)))], dtype=np.float32)
    tilted = np.concatenate([tilted, [[np.nan, 0, -1], [0, 0, np.inf]]]).astype(np.float32)
    four = np.repeat(centre, 5, axis=0)
    idx, _, _ = one_step(four, target, normals, 3, 3, DYADIC_K, np.eye(4), 0.25, source_normals=tilted, min_cos=0.5)
    want, _ = pref.correspond_projective(four, target, normals, 3, 3, DYADIC_K, np.eye(4), 0.25, source_normals=tilted, min_cos=0.5)
    assert idx.tolist() == want.tolist() == [4, -1, 4, -1, -1]
    # min_cos itself is rounded once to float32: 0.5 + 2^-26 is 0.5 there
    assert one_step(four, target, normals, 3, 3, DYADIC_K, np.eye(4), 0.25, source_normals=tilted, min_cos=0.5 + 2.0 ** -26)[0].tolist() == [4, -1, 4, -1, -1]
    # the gate off: the source's normals are not looked at, and need not be there
    assert one_step(four, target, normals, 3, 3, DYADIC_K, np.eye(4), 0.25, source_normals=tilted)[0].tolist() == [4] * 5
    assert one_step(four, target, normals, 3, 3, DYADIC_K, np.eye(4), 0.25)[0].tolist() == [4] * 5
    # the gate turns the SOURCE's normal by the pose: a quarter turn about x takes (0, 1, 0) to (0, 0, 1) and (0, -1, 0) to (0, 0, -1)
    turn = np.eye(4)
    turn[:3, :3] = [[1, 0, 0], [0, 0, -1], [0, 1, 0]]
    turn[:3, 3] = [0, 0, 1]
    flat_source = np.array([[0, 0, 0], [0, 0, 0]], dtype=np.float32)
    idx, _, _ = one_step(flat_source, target, normals, 3, 3, DYADIC_K, turn, 0.25, source_normals=[[0, -1, 0], [0, 1, 0]], min_cos=0.5)
    want, _ = pref.correspond_projective(flat_source, target, normals, 3, 3, DYADIC_K, turn, 0.25, source_normals=[[0, -1, 0], [0, 1, 0]],
                                         min_cos=0.5)
    assert idx.tolist() == want.tolist() == [4, -1]


@pytest.fixture(scope="module")
def corner():
    """The rendered corner, its normals by the restatement, and the restatement's registrations (gate off, 30 degrees)."""
    target, source, truth = corner_views()
    nt = pref.image_normals(target, CORNER_W, CORNER_H, CORNER_STEP, 0.02)
    ns = pref.image_normals(source, CORNER_W, CORNER_H, CORNER_STEP, 0.02)
    restated = {angle: pref.icp_projective(source, target, nt, CORNER_W, CORNER_H, CORNER_K, None,
                                           {"max_dist": 0.02, "min_cos": pref.min_cos(angle)}, ns) for angle in (None, 30.0)}
    return target, source, truth, nt, ns, restated


@pytest.mark.parametrize("stride", [1, 2, 5])
def test_strides_and_a_pose_that_is_no_lattice_motion(corner, stride):
    target, source, _, nt, ns, _ = corner
    for pose in (np.eye(4), ref.perturbation(1.0, 3.0)):
        for min_cos in (None, math.cos(math.radians(30.0))):
            idx, sums, _ = one_step(source, target, nt, CORNER_W, CORNER_H, CORNER_K, pose, 0.02, stride=stride, source_normals=ns,
                                    min_cos=min_cos)
            want, _ = pref.correspond_projective(source, target, nt, CORNER_W, CORNER_H, CORNER_K, pose, 0.02, stride=stride,
                                                 source_normals=ns, min_cos=min_cos)
            assert len(idx) == -(-len(source) // stride) and idx.tolist() == want.tolist()
            assert sums[28] == float((want >= 0).sum()) > 200 and (want == -2).any() and (want == -1).any()


def test_sums_pair_count_exact_floats_within_the_rounding_of_their_sum_and_reproducible(corner):
    target, source, _, nt, ns, _ = corner
    run = lambda: one_step(source, target, nt, CORNER_W, CORNER_H, CORNER_K, np.eye(4), 0.02, source_normals=ns, min_cos=0.5)   # noqa: E731
    idx, sums, state = run()
    want_idx, p = pref.correspond_projective(source, target, nt, CORNER_W, CORNER_H, CORNER_K, np.eye(4), 0.02, source_normals=ns,
                                             min_cos=0.5)
    want, terms = ref.sums(p, target, nt, want_idx)
    assert idx.tolist() == want_idx.tolist() and sums[28] == want[28] > 1000
    # the terms are the same IEEE operations on both sides; fsum is their exact sum rounded once; a float64 sum of n terms in
    # any order is within (n - 1) u / (1 - (n - 1) u) of it times the sum of magnitudes (Higham, Accuracy and Stability, 4.2)
    n = len(terms)
    for c in range(28):
        magnitude = math.fsum(np.abs(terms[:, c]))
        bound = (n - 1) * U / (1.0 - (n - 1) * U) * magnitude + U * abs(want[c])
        print("sum %2d: device %+.17e  reference %+.17e  |diff| %.3e  bound %.3e" % (c, sums[c], want[c], abs(sums[c] - want[c]), bound))
        assert abs(sums[c] - want[c]) <= bound, c
    idx2, sums2, state2 = run()
    assert sums2.tobytes() == sums.tobytes() and state2.tobytes() == state.tobytes() and idx2.tobytes() == idx.tobytes()


@pytest.mark.parametrize("angle", [None, 30.0])
def test_the_loop_on_the_rendered_corner(corner, angle):
    from regnet_for_3d_grasping_amd import depth_frame, registration
    target, source, truth, nt, ns, restated = corner
    want = restated[angle]
    params = {"max_dist": 0.02, "association": "projective", "normal_angle": angle, "normal_step": CORNER_STEP}
    tgt = registration.prepare_projective_target(gpu(target), CORNER_W, CORNER_H, CORNER_K, params)
    assert tgt.normals.cpu().numpy().tobytes() == depth_frame.normals(gpu(target), CORNER_W, CORNER_H, CORNER_STEP, 0.02).cpu().numpy().tobytes()
    assert np.array_equal(tgt.normals.cpu().numpy(), nt, equal_nan=True)
    reg = registration.icp(gpu(source), tgt, None, params, source_shape=(CORNER_W, CORNER_H))
    e_ref, e_gpu = ref.pose_distance(want["pose"], truth), ref.pose_distance(reg.pose(), truth)
    floor = corner_floor(target, 0.02)
    print("device: status %d, %d iterations, pairs %d, rms %.3g -> %.3g, error %.3g; restatement: %d iterations, error %.3g; floor %.3g"
          % (reg.status, reg.iterations, reg.pairs, reg.rms_first, reg.rms_last, e_gpu, want["iterations"], e_ref, floor))
    assert reg.status == registration.CONVERGED == want["status"]
    assert reg.iterations == want["iterations"] and reg.pairs == want["pairs"]
    assert reg.result()["history"][:, 0].tolist() == want["history"][:, 0].tolist()
    assert e_gpu <= max(2 * e_ref, floor)
    # steps enqueued after CONVERGED change nothing, byte for byte: not the state, not the outputs
    before = reg.state.cpu().numpy().tobytes()
    idx, sums, after = one_step(source, target, nt, CORNER_W, CORNER_H, CORNER_K, None, 0.02, source_normals=ns,
                                min_cos=pref.min_cos(angle), state=reg.state)
    assert after.tobytes() == before and (idx == -9).all() and np.isnan(sums).all()
    # the source's normals given, and a side stream: the same bytes
    side = torch.cuda.Stream(device=DEV)
    src, given = gpu(source), gpu(ns)
    torch.cuda.synchronize()
    other = registration.icp(src, tgt, None, params, source_normals=given, stream=side)
    side.synchronize()
    assert other.state.cpu().numpy().tobytes() == before


def test_too_few_keeps_the_pose_and_fit_normals_run(corner):
    from regnet_for_3d_grasping_amd import registration
    target, source, truth, nt, _, _ = corner
    params = {"max_dist": 0.02, "association": "projective", "normal_step": CORNER_STEP}
    tgt = registration.prepare_projective_target(gpu(target), CORNER_W, CORNER_H, CORNER_K, params, target_normals=gpu(nt))
    off = np.array(truth)
    off[:3, 3] += 5.0
    lost = registration.icp(gpu(source), tgt, off, params)
    assert lost.status == registration.TOO_FEW and lost.iterations == 1 and lost.pairs == 0 and lost.pose().tobytes() == off.tobytes()
    empty = registration.icp(gpu(np.zeros((0, 3), dtype=np.float32)), tgt, None, params)
    assert empty.status == registration.TOO_FEW and empty.pairs == 0
    # "fit": estimate_normals on the finite rows, scattered back -- NaN exactly where the cloud is, unit length elsewhere
    fit = registration.organised_normals(gpu(target), CORNER_W, CORNER_H, dict(params, normals="fit", normal_radius=0.06)).cpu().numpy()
    finite = np.isfinite(target).all(axis=1)
    assert np.isnan(fit[~finite]).all() and np.allclose(np.linalg.norm(fit[finite], axis=1), 1.0, atol=1e-5)
    assert (np.einsum("ij,ij->i", fit[finite], target[finite]) <= 0).all()                 # facing the camera


def test_nearest_on_the_same_inputs_gives_the_same_bytes_twice_through_the_shared_tail():
    from regnet_for_3d_grasping_amd import registration
    target, normals = ref.corner_scene()
    source = ref.moved_source(target, ref.perturbation(2.5, 7.0))
    tgt = registration.prepare_target(gpu(target), {"max_dist": 0.02}, gpu(normals))
    runs = []
    for _ in range(2):
        state = gpu(registration.initial_state(None, None))
        idx = torch.full((len(source),), -9, dtype=torch.int32, device=DEV)
        sums = torch.full((29,), float("nan"), dtype=torch.float64, device=DEV)
        registration.step(gpu(source), tgt, state, {"max_dist": 0.02}, idx, sums)
        runs.append((idx.cpu().numpy(), sums.cpu().numpy(), state.cpu().numpy()))
    assert all(a.tobytes() == b.tobytes() for a, b in zip(*runs))
    want_idx, p = ref.correspond(source, target, np.eye(4), 0.02)
    back = tgt.rows.cpu().numpy()
    assert back[runs[0][0]].tolist() == want_idx.tolist() and runs[0][1][28] == 575.0
    want, terms = ref.sums(p, target, normals, want_idx)
    n = len(terms)
    for c in range(28):
        assert abs(runs[0][1][c] - want[c]) <= (n - 1) * U / (1.0 - (n - 1) * U) * math.fsum(np.abs(terms[:, c])) + U * abs(want[c]), c


def test_every_new_error_code_and_the_python_refusals(corner):
    from regnet_for_3d_grasping_amd import _lib, registration
    target, source, _, nt, ns, _ = corner
    src, tgt, nrm, sn = gpu(source), gpu(target), gpu(nt), gpu(ns)
    state = gpu(registration.initial_state(None, None))
    ws = torch.empty((registration.projective_workspace_bytes(len(source)),), dtype=torch.uint8, device=DEV)
    k = np.array(CORNER_K, dtype=np.float64)
    stream = torch.cuda.current_stream().cuda_stream

    def call(**change):
        a = dict(source=src.data_ptr(), n=len(source), stride=1, sn=sn.data_ptr(), target=tgt.data_ptr(), normals=nrm.data_ptr(), W=CORNER_W,
                 H=CORNER_H, k=k.ctypes.data, window=1, state=state.data_ptr(), max_dist=0.02, min_cos=0.5, idx=None, sums=None,
                 min_pairs=0, ws=ws.data_ptr())
        a.update(change)
        return _lib.lib.regnet_icp_step_projective_f32(*a.values(), stream)

    assert call() == 0 and call(sn=None, min_cos=-1.5) == 0
    shape = call(window=3)
    assert shape != 0 and all(call(**bad) == shape for bad in ({"window": -1}, {"n": -1}, {"W": 0}, {"H": 0}, {"stride": 0}, {"min_pairs": -1}))
    unsupported = call(min_cos=1.5)
    assert unsupported not in (0, shape)
    bad_k = [np.array(v, dtype=np.float64) for v in ((0.0, 60, 31.5, 23.5), (60, -1.0, 31.5, 23.5), (float("nan"), 60, 31.5, 23.5),
                                                     (60, float("inf"), 31.5, 23.5), (1e60, 60, 31.5, 23.5), (60, 1e-60, 31.5, 23.5))]
    for bad in ([{"min_cos": float("nan")}, {"min_cos": float("inf")}, {"n": (1 << 21) + 1}, {"W": 1 << 11, "H": (1 << 10) + 1},
                 {"max_dist": 0.0}, {"max_dist": float("nan")}] + [{"k": v.ctypes.data} for v in bad_k]):
        assert call(**bad) == unsupported, bad
    null = call(sn=None)                                                      # the gate is on: the source's normals are required
    assert null not in (0, shape, unsupported)
    assert all(call(**{name: None}) == null for name in ("source", "target", "normals", "k", "state", "ws"))
    assert call(source=None, n=0) == 0                                        # no source row: launch B alone
    torch.cuda.synchronize()
    # Python
    projective = {"max_dist": 0.02, "association": "projective"}
    prepared = registration.prepare_projective_target(tgt, CORNER_W, CORNER_H, CORNER_K, projective, target_normals=nrm, max_source=100)
    nearest = registration.prepare_target(tgt, {"max_dist": 0.02}, torch.nan_to_num(nrm))
    with pytest.raises(ValueError, match="ProjectiveTarget"):
        registration.icp(src, tgt, None, projective)
    with pytest.raises(ValueError, match="association='projective'"):
        registration.icp(src, prepared, None, {"max_dist": 0.02})
    with pytest.raises(ValueError, match="100 source rows"):
        registration.icp(src, prepared, None, projective)
    with pytest.raises(ValueError, match="source_shape"):
        registration.icp(src[:100].contiguous(), prepared, None, dict(projective, normal_angle=30.0))
    with pytest.raises(ValueError, match="does not go with"):
        registration.step(src[:100].contiguous(), nearest, state, projective)
    with pytest.raises(ValueError, match="does not go with"):
        registration.step(src[:100].contiguous(), prepared, state, {"max_dist": 0.02})
    with pytest.raises(ValueError, match="source_normals"):
        registration.step(src[:100].contiguous(), prepared, state, dict(projective, normal_angle=30.0))
    with pytest.raises(ValueError, match="width \\* height"):
        registration.prepare_projective_target(tgt, CORNER_W, CORNER_H - 1, CORNER_K, projective)
    with pytest.raises(ValueError, match="intrinsics"):
        registration.prepare_projective_target(tgt, CORNER_W, CORNER_H, (0.0, 60.0, 1.0, 1.0), projective)
    with pytest.raises(ValueError, match="rows"):
        registration.prepare_projective_target(tgt, CORNER_W, CORNER_H, CORNER_K, projective, target_normals=nrm[:5])
    with pytest.raises(RuntimeError, match="CUDA"):
        registration.prepare_projective_target(tgt.cpu(), CORNER_W, CORNER_H, CORNER_K, projective)
