"""Approach analysis against the TSDF volume on the MI355X (csrc/approach_volume.hip through approach_volume.py) against the numpy
restatement of the contract (tests/approach_volume_reference.py).  Every comparison is exact, counts and values: the contract is
fp32 multiply, add, divide, floor, compare, min and max in a fixed order, and integer counts.  The restatement is fed the
local-to-volume rows the device computed (downloaded): the kernel takes them as an input, so no sin / cos and no float64 product
sits inside what is compared.  Volumes are set by hand through ``Volume.D`` / ``Volume.W`` where a rule needs it."""
import functools

import numpy as np
import pytest
import torch

from . import approach_reference as cloud_ref
from . import approach_volume_reference as ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
f32 = np.float32
inf = float("inf")
WIDTH, DEPTH = 0.08, 0.06
GRIPPER = ref.gripper_box(DEPTH, WIDTH)
DYADIC_BOX = (-0.5, 0.5, 0.125, 1.0, 0.75, 0.0)
IDENTITY_L = np.eye(4, dtype=np.float32)[:3].reshape(1, 12)
SENTINEL = -77


def _dev(a, dtype=np.float32):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(DEV)


def _volume(hand):
    """A ``ref.HandVolume`` -> the ``tsdf.Volume`` holding its planes."""
    from regnet_for_3d_grasping_amd import tsdf
    vol = tsdf.Volume(tsdf.TsdfParams(voxel=hand.voxel, trunc=hand.trunc, origin=tuple(float(v) for v in hand.origin), dims=hand.dims,
                                      min_weight=hand.min_weight, max_points=1 << 14), DEV)
    vol.D.copy_(_dev(hand.D))
    vol.W.copy_(_dev(hand.W, np.int32))
    return vol


def _kernel(vol, L, box, standoff, step, x_extent, margin=0.0, out=None):
    """The C entry point on a ``tsdf.Volume`` -> (counts, values) as numpy arrays.  The outputs are the middle rows of guarded
    buffers: a row of sentinels before and after them must survive."""
    from regnet_for_3d_grasping_amd import _lib
    p = vol.params
    L = _dev(L)
    B = int(L.shape[0])
    x_lo, x_hi, ht, hw, hs, back_x = box
    per = _dev(x_hi) if np.ndim(x_hi) else None
    counts = torch.full((B + 2, 8), SENTINEL, dtype=torch.int32, device=DEV)
    values = torch.full((B + 2, 4), float(SENTINEL), dtype=torch.float32, device=DEV)
    _lib.call("regnet_grasp_approach_volume_f32", vol.data, vol.data.data_ptr(), *p.dims, vol.origin.ctypes.data, float(p.voxel),
              float(p.trunc), int(p.min_weight), float(margin), L.data_ptr(), B, float(x_lo), 0.0 if per is not None else float(x_hi),
              None if per is None else per.data_ptr(), float(ht), float(hw), float(hs), float(back_x), float(standoff), float(step),
              float(x_extent), counts[1:].data_ptr(), values[1:].data_ptr())
    counts, values = counts.cpu().numpy(), values.cpu().numpy()
    assert (counts[[0, -1]] == SENTINEL).all() and (values[[0, -1]] == SENTINEL).all()
    return counts[1:-1], values[1:-1]


def _same(got, want, what=""):
    assert got[0].dtype == np.int32 and got[1].dtype == np.float32
    assert np.array_equal(got[0], want[0]), (what, got[0], want[0])
    assert got[1].tobytes() == want[1].tobytes(), (what, got[1], want[1])


def _both(hand, L, box, standoff, step, x_extent, margin=0.0):
    """Device and restatement on one hand-built volume, held equal -> (counts, values)."""
    got = _kernel(_volume(hand), L, box, standoff, step, x_extent, margin)
    _same(got, hand.run(L, box, standoff, step, x_extent, margin), (standoff, step, margin))
    return got


# ---- random volumes, random grasps, through analyse_volume ------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _random_volume(min_weight=2):
    """Ragged dims.  Seen free (D in (0, 1], many exactly 1) with a solid floor below z = -4 cm, a never-observed quarter
    (x > 3 cm, W in 0..1 below min_weight = 2), and speckles all over: solid ones, NaN distances, low weights."""
    rng = np.random.default_rng(40)
    hand = ref.HandVolume((40, 36, 33), (-0.1, -0.09, -0.08), 0.005, trunc=0.02, min_weight=min_weight)
    n = hand.D.shape
    ix, iz = np.arange(n[0]) % 40, np.arange(n[0]) // (40 * 36)
    hand.D[:] = np.where(rng.uniform(size=n) < 0.5, 1.0, rng.uniform(0.01, 1, n))
    hand.W[:] = rng.integers(2, 4, n)
    hand.D[iz < 8] = rng.uniform(-1, -0.01, n)[iz < 8]
    hand.W[ix >= 26] = rng.integers(0, 2, n)[ix >= 26]
    speckle = rng.uniform(size=n)
    hand.D[speckle < 0.0005] = -0.3
    hand.D[(speckle > 0.0005) & (speckle < 0.001)] = np.nan
    hand.W[(speckle > 0.001) & (speckle < 0.0015)] = 1
    return hand, _volume(hand)


TURNED = np.array([[0.36, 0.48, -0.8, 0.01], [-0.8, 0.6, 0.0, -0.02], [0.48, 0.64, 0.6, 0.015], [0, 0, 0, 1.0]])   # a rotation


def _analyse_and_check(B, depth, standoff, step, to_volume=None, max_depth=None, margin=0.0, unseen="free", **kw):
    from regnet_for_3d_grasping_amd import approach
    hand, vol = _random_volume()
    grasp = _dev(cloud_ref.random_grasps(np.random.default_rng(B), max(B, 1), spread=0.05)[:B])
    params = approach.ApproachParams(standoff=standoff, step=step, margin=margin, unseen=unseen, **kw)
    res = approach.analyse_volume(vol, grasp, depth, WIDTH, params, to_volume=to_volume, max_depth=max_depth)
    assert isinstance(res, approach.VolumeApproach)
    assert res.counts.shape == (B, 8) and res.counts.dtype == torch.int32 and res.values.shape == (B, 4) and res.L.shape == (B, 12)
    host_depth = depth.cpu().numpy() if isinstance(depth, torch.Tensor) else depth
    box = ref.gripper_box(host_depth, WIDTH)
    extent = max_depth if max_depth is not None else depth
    want = hand.run(res.L.cpu().numpy(), box, standoff, hand.voxel if step is None else step, extent, margin)
    _same((res.counts.cpu().numpy(), res.values.cpu().numpy()), want, (B, standoff, step))
    assert res.samples == ref.lattice_counts(box, standoff, hand.voxel if step is None else step, extent)[0]
    # L is to_volume @ [frame | centre] up to the one rounding
    frame, center = res.frame.cpu().numpy(), res.center.cpu().numpy()
    assert np.abs(res.L.cpu().numpy() - ref.rows_of(frame, center, to_volume)).max() <= 2.0 ** -22
    derived = ref.derived_ref(want[0], want[1], frame, center, params.pad, box[4], unseen)
    got = {"grasp_clearance": res.clearance, "grasp_width": res.width, "grasp_offset": res.offset, "grasp_opening": res.opening,
           "grasp_contact": res.contact, "grasp_pregrasp": res.pregrasp, "grasp_clearance_seen": res.clearance_seen,
           "grasp_clearance_safe": res.clearance_safe, "grasp_unseen": res.unseen_share, "grasp_solid_hand": res.solid_hand}
    for key, value in derived.items():
        assert got[key].cpu().numpy().dtype == value.dtype and got[key].cpu().numpy().tobytes() == value.tobytes(), key
    assert np.array_equal(res.passes().cpu().numpy(), ref.passes_ref(derived, params.min_clearance, params.min_contact))
    return res, want, derived


@pytest.mark.parametrize("B", [1, 3, 67])
def test_random_volume_and_grasps(B):
    # step 3 mm: 54 x 34 x 4 samples (7 x 5 tiles, the last ones partial); the voxel (None): 32 x 21 x 2; 7 mm with S = 0
    _, want, _ = _analyse_and_check(B, DEPTH, 0.1, 0.003)
    assert want[0][:, :6].any(axis=0).all() and (want[0][:, 7] < want[0][:, 6]).all()          # not vacuous: every class met
    _analyse_and_check(B, DEPTH, 0.1, None, margin=0.004)
    _analyse_and_check(B, DEPTH, 0.0, 0.007)
    _analyse_and_check(B, DEPTH, 0.05, 0.004, to_volume=TURNED)
    per = _dev(np.random.default_rng(B).uniform(0.03, 0.08, B))
    _, want, _ = _analyse_and_check(B, per, 0.05, 0.004, max_depth=0.08)
    if B == 67:
        assert len(np.unique(want[0][:, 6])) > 5                                                # the depths are honoured per grasp


def test_both_policies_and_the_filters():
    _, _, free = _analyse_and_check(67, DEPTH, 0.1, 0.004, min_clearance=0.03)
    _, _, blocked = _analyse_and_check(67, DEPTH, 0.1, 0.004, unseen="blocked", min_clearance=0.03)
    assert (blocked["grasp_clearance"] <= free["grasp_clearance"]).all() and (blocked["grasp_clearance"] < free["grasp_clearance"]).any()
    assert ref.passes_ref(free, 0.03).sum() > ref.passes_ref(blocked, 0.03).sum()
    from regnet_for_3d_grasping_amd import approach
    hand, vol = _random_volume()
    with pytest.raises(ValueError, match="max_depth"):
        approach.analyse_volume(vol, torch.zeros((2, 8), device=DEV), torch.full((2,), 0.05, device=DEV), WIDTH)
    with pytest.raises(ValueError, match="2\\^22"):
        approach.analyse_volume(vol, torch.zeros((2, 8), device=DEV), DEPTH, WIDTH, {"step": 1e-4})


# ---- one hand-built volume per rule -------------------------------------------------------------------------------------------------
def _dyadic(min_weight=1):
    return ref.HandVolume((6, 8, 1), (-1.0, -1.0, -0.125), 0.25, trunc=1.0, min_weight=min_weight)


def _at(vol, x, y):
    return vol.at(int((x + 1.0) / 0.25), int((y + 1.0) / 0.25), 0)


def _dy(hand, margin=0.0, L=IDENTITY_L, box=DYADIC_BOX, standoff=0.5, step=0.25):
    counts, values = _both(hand, L, box, standoff, step, 0.5, margin)
    return counts[0].tolist(), values[0].tolist()


def test_classification_rules_on_hand_set_volumes():
    assert _dy(_dyadic().observe_all(1.0)) == ([0, 0, 0, 0, 0, 0, 60, 0], [inf, -inf, 0.5, 0.5])      # D == 1 is FREE
    assert _dy(_dyadic()) == ([0, 24, 0, 24, 0, 36, 60, 0], [inf, -inf, 0.5, 0.0])                     # never observed
    assert _dy(_dyadic().observe_all(-0.5)) == ([24, 0, 24, 0, 36, 0, 60, 0], [-0.625, 0.625, 0.0, 0.0])
    # D at d_solid and one ulp either side, margin 0 and positive (trunc = 1: d_solid = margin); -0.0 is not below 0
    for margin, d_solid in ((0.0, f32(0.0)), (0.25, f32(0.25))):
        seen = []
        for d in (np.nextafter(d_solid, f32(-np.inf)), d_solid, np.nextafter(d_solid, f32(np.inf)), f32(-0.0) if margin == 0 else d_solid):
            hand = _dyadic().observe_all(1.0)
            hand.D[_at(hand, -0.875, 0.125)] = d
            counts, values = _dy(hand, margin=margin)
            seen.append((counts[4], values[2]))
        assert seen == [(1, 0.375), (0, 0.5), (0, 0.5), (0, 0.5)], (margin, seen)
    # W at min_weight - 1 and at min_weight; a NaN distance is UNKNOWN
    for mw in (1, 2, 3):
        for w, d, expected in ((mw - 1, -1.0, ([0, 0, 0, 0, 0, 1, 60, 0], [inf, -inf, 0.5, 0.125])),
                               (mw, -1.0, ([0, 0, 0, 0, 1, 0, 60, 0], [inf, -inf, 0.125, 0.125])),
                               (mw, np.nan, ([0, 0, 0, 0, 0, 1, 60, 0], [inf, -inf, 0.5, 0.125]))):
            hand = _dyadic(mw).observe_all(1.0, w=mw)
            hand.D[_at(hand, -0.625, -0.375)], hand.W[_at(hand, -0.625, -0.375)] = f32(d), w
            assert _dy(hand) == expected, (mw, w, d)


def test_faces_nan_rows_a_far_volume_and_one_sample_per_axis():
    free = _dyadic().observe_all(1.0)
    for dx, outside in ((-0.125, 0), (-0.375, 8), (0.0625, 0), (0.125, 4)):      # index 0 ON the low face, -1, n - 1, n ON the high face
        row = IDENTITY_L.copy()
        row[0, 3] = dx
        assert _dy(free, L=row)[0][7] == outside, dx
    for dy, outside in ((-0.125, 0), (-0.375, 12), (0.125, 12)):                # the same along y: a lane's 6 samples leave (2 back, 4 finger, 6 blockers)
        row = IDENTITY_L.copy()
        row[0, 7] = dy
        assert _dy(free, L=row)[0][7] == outside, dy
    far = IDENTITY_L.copy()
    far[0, 7] = 100.0                                                            # a volume wholly outside the hand
    everything_outside = ([0, 24, 0, 24, 0, 36, 60, 60], [inf, -inf, 0.5, 0.0])
    assert _dy(free, L=far) == everything_outside
    rows = np.repeat(IDENTITY_L, 4, axis=0)                                      # a grasp row with NaN / inf entries: all OUTSIDE
    rows[1, 5], rows[2, 0], rows[3, 11] = np.nan, np.inf, -np.inf
    counts, values = _both(free, rows, DYADIC_BOX, 0.5, 0.25, 0.5)
    assert counts[0].tolist() == [0, 0, 0, 0, 0, 0, 60, 0]
    for b in (1, 2, 3):
        assert (counts[b].tolist(), values[b].tolist()) == everything_outside
    # h larger than the box: one sample per axis, at (xs + 4, 4 - hw, 4 - ht): in nothing, nothing is looked up
    assert _dy(free, step=8.0) == ([0] * 8, [inf, -inf, 0.5, 0.5])
    # one sample per axis that IS in a set: S = 0, h = 1: x = 0, y = 0.5 - 1 = -0.5, z = 0.375: |z| >= ht, in nothing either; h = 0.25
    # with a thick hand: a lattice of 4 x 8 x 4
    thick = (-0.5, 0.5, 0.5, 1.0, 0.75, 0.0)
    tall = ref.HandVolume((6, 8, 4), (-1.0, -1.0, -0.5), 0.25, trunc=1.0).observe_all(-0.5)
    counts, _ = _both(tall, IDENTITY_L, thick, 0.0, 0.25, 0.5)
    assert counts[0].tolist() == [96, 0, 96, 0, 80, 0, 176, 0]


def test_per_grasp_depth_no_standoff_and_no_grasp():
    solid = _dyadic().observe_all(-0.5)
    box = (-0.5, np.array([0.5, 0.125], dtype=np.float32), 0.125, 1.0, 0.75, 0.0)
    counts, values = _both(solid, np.repeat(IDENTITY_L, 2, axis=0), box, 0.5, 0.25, 0.5)
    assert counts.tolist() == [[24, 0, 24, 0, 36, 0, 60, 0], [12, 0, 20, 0, 32, 0, 52, 0]]
    counts, values = _both(solid, IDENTITY_L, DYADIC_BOX, 0.0, 0.25, 0.5)
    assert counts[0].tolist() == [24, 0, 24, 0, 20, 0, 44, 0] and values[0].tolist() == [-0.625, 0.625, 0.0, 0.0]
    _, values = _both(_dyadic().observe_all(1.0), IDENTITY_L, DYADIC_BOX, 0.0, 0.25, 0.5)
    assert values[0].tolist() == [inf, -inf, 0.0, 0.0] and not np.signbit(values[0, 2:]).any()      # -0.0 never leaves the kernel
    counts, values = _kernel(_volume(solid), np.zeros((0, 12), dtype=np.float32), DYADIC_BOX, 0.5, 0.25, 0.5)   # B == 0
    assert counts.shape == (0, 8) and values.shape == (0, 4)


# ---- reductions: the deciding sample in every wave and in the partial tiles ---------------------------------------------------------
@pytest.mark.parametrize("i,j", [(3, 5), (12, 5), (2, 12), (20, 18), (26, 19), (27, 2), (21, 10)])
def test_the_deciding_sample_is_found_in_every_wave(i, j):
    """The reference's gripper at a 5 mm step: 28 x 21 x 2 samples, 4 x 3 tiles of 8 x 8, tile t = 4 ty + tx on wave t % 4; the
    columns i >= 24 and the rows j >= 16 are partial tiles.  One solid voxel at sample (i, j) decides a minimum or a maximum."""
    hand = ref.HandVolume((60, 40, 20), (-0.2, -0.1, -0.05), 0.005, trunc=0.02).observe_all(1.0)
    plain = _both(hand, IDENTITY_L, GRIPPER, 0.02, 0.005, DEPTH)
    assert plain[0][0].tolist() == [0, 0, 0, 0, 0, 0, plain[0][0, 6], 0] and plain[1][0].tolist() == [inf, -inf, f32(0.02), f32(0.02)]
    xv, yv, zv = ref.lattice_samples(GRIPPER, 0.02, 0.005, DEPTH)
    c = [int(np.floor((f32(v) - f32(o)) / f32(0.005))) for v, o in ((xv[i], -0.2), (yv[j], -0.1), (zv[1], -0.05))]
    hand.D[hand.at(*c)] = f32(-0.25)
    counts, values = _both(hand, IDENTITY_L, GRIPPER, 0.02, 0.005, DEPTH)
    x, y = xv[i], yv[j]
    if abs(y) < 0.04 and x > 0:                                                   # between the fingers
        assert counts[0, 0] == 1 and values[0, 0] == y and values[0, 1] == y
    else:                                                                         # behind the palm's face or in a finger lane
        assert counts[0, 4] == 1 and values[0, 2] == max(f32(-0.06) - x, f32(0.0)) == values[0, 3]


# ---- streams, graphs, repeatability -------------------------------------------------------------------------------------------------
def test_side_stream_graph_replay_and_two_runs_give_the_same_bytes():
    from regnet_for_3d_grasping_amd import approach
    hand, vol = _random_volume()
    params = approach.ApproachParams(standoff=0.05, step=0.004, unseen="blocked", min_clearance=0.01)
    grasps = [_dev(cloud_ref.random_grasps(np.random.default_rng(s), 67, spread=0.05)) for s in (1, 2)]
    grasp = grasps[0].clone()
    depth = torch.full((67,), DEPTH, device=DEV)

    def run():
        res = approach.analyse_volume(vol, grasp, depth, WIDTH, params, max_depth=DEPTH)
        return res, (res.counts, res.values, res.clearance, res.pregrasp, res.unseen_share, res.passes())

    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        a, _ = run()
        b, _ = run()
    side.synchronize()
    torch.cuda.current_stream(DEV).wait_stream(side)
    want = hand.run(a.L.cpu().numpy(), GRIPPER, 0.05, 0.004, DEPTH)
    for res in (a, b):
        _same((res.counts.cpu().numpy(), res.values.cpu().numpy()), want)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        _, outputs = run()
    replayed = []
    for g in (grasps[0], grasps[1], grasps[0]):
        outputs[0].fill_(SENTINEL)
        outputs[1].fill_(SENTINEL)
        grasp.copy_(g)
        graph.replay()
        torch.cuda.synchronize()
        _, eager = run()
        for got, ref_t in zip(outputs, eager):
            assert got.cpu().numpy().tobytes() == ref_t.cpu().numpy().tobytes()
        replayed.append(outputs[0].clone())
    assert torch.equal(replayed[0], a.counts) and torch.equal(replayed[2], a.counts) and not torch.equal(replayed[1], a.counts)


# ---- the ABI's errors: before any launch ----------------------------------------------------------------------------------------------
def test_every_error_code_leaves_the_outputs_alone():
    from regnet_for_3d_grasping_amd import _lib
    hand = _dyadic().observe_all(-0.5)
    vol = _volume(hand)
    L = _dev(np.repeat(IDENTITY_L, 2, axis=0))
    counts = torch.full((2, 8), SENTINEL, dtype=torch.int32, device=DEV)
    values = torch.full((2, 4), float(SENTINEL), dtype=torch.float32, device=DEV)
    stream = torch.cuda.current_stream(DEV).cuda_stream

    def raw(volume=vol.data.data_ptr(), dims=(6, 8, 1), origin3=vol.origin.ctypes.data, voxel=0.25, trunc=1.0, min_weight=1, margin=0.0,
            l=L.data_ptr(), B=2, standoff=0.5, step=0.25, x_extent=0.5, c=counts.data_ptr(), v=values.data_ptr()):
        return _lib.lib.regnet_grasp_approach_volume_f32(volume, dims[0], dims[1], dims[2], origin3, voxel, trunc, min_weight, margin, l, B,
                                                         -0.5, 0.5, None, 0.125, 1.0, 0.75, 0.0, standoff, step, x_extent, c, v, stream)

    assert raw(B=-1) == -1 and raw(dims=(0, 8, 1)) == -1 and raw(dims=(6, 8, -1)) == -1 and raw(min_weight=0) == -1
    assert raw(dims=(1 << 10, 1 << 10, 1 << 9)) == -3 and raw(dims=((1 << 24) + 1, 1, 1)) == -3
    for name in ("voxel", "trunc", "step"):
        for bad in (0.0, -1.0, float("nan"), float("inf")):
            assert raw(**{name: bad}) == -3, (name, bad)
    assert raw(standoff=-1e-3) == -3 and raw(standoff=float("nan")) == -3 and raw(standoff=float("inf")) == -3
    assert raw(margin=float("nan")) == -3 and raw(step=2.0 ** -12, x_extent=3.0) == -3 and raw(x_extent=float("nan")) == -3
    for null in ("volume", "origin3", "l", "c", "v"):
        assert raw(**{null: None}) == -2, null
    assert raw(B=0) == 0 and raw(B=0, volume=None) == 0                     # nothing to do: no launch
    torch.cuda.synchronize()
    assert (counts == SENTINEL).all() and (values == float(SENTINEL)).all()
    with pytest.raises(RuntimeError, match="regnet_grasp_approach_volume_f32 failed"):
        _kernel(vol, IDENTITY_L, DYADIC_BOX, -1.0, 0.25, 0.5)
    assert raw() == 0
    torch.cuda.synchronize()
    assert counts.tolist() == [[24, 0, 24, 0, 36, 0, 60, 0]] * 2 and values.tolist() == [[-0.625, 0.625, 0.0, 0.0]] * 2


# ---- the contact pass on the model's own normals ----------------------------------------------------------------------------------------
def test_contact_from_the_surface_of_a_device_integrated_volume():
    """Two rendered views of a box on a table are integrated on the device; the contact counts of ``analyse_volume`` equal
    ``approach_reference`` fed the extracted surface's rows and normals and the T the device formed."""
    from regnet_for_3d_grasping_amd import approach, tsdf
    from .icp_projective_reference import look_at, rectangle, render
    W, H, K = 128, 96, (120.0, 120.0, 63.5, 47.5)
    x, y, t = 0.03, 0.03, 0.06
    scene = [rectangle((-0.5, -0.5, 0.0), (1.0, 0, 0), (0, 1.0, 0)), rectangle((-x, -y, t), (2 * x, 0, 0), (0, 2 * y, 0)),
             rectangle((-x, -y, 0.0), (2 * x, 0, 0), (0, 0, t)), rectangle((-x, y, 0.0), (2 * x, 0, 0), (0, 0, t)),
             rectangle((-x, -y, 0.0), (0, 2 * y, 0), (0, 0, t)), rectangle((x, -y, 0.0), (0, 2 * y, 0), (0, 0, t))]
    vol = tsdf.Volume(tsdf.TsdfParams(voxel=0.005, trunc=0.01, origin=(-0.12, -0.10, -0.015), dims=(48, 40, 36), max_points=1 << 13), DEV)
    for eye in ((0.0, -0.35, 0.30), (0.0, 0.35, 0.30)):
        pose = look_at(eye, (0.0, 0.0, 0.03))
        vol.integrate((_dev(render(scene, W, H, K, pose)), None, W, H, K), pose)
    surface = vol.extract()
    k, _, _ = surface.check()
    assert 500 < k < (1 << 13)
    grasp = np.zeros((3, 8), dtype=np.float32)
    grasp[:, :3] = [(0.0, 0.0, 0.08), (0.004, 0.003, 0.085), (0.0, 0.0, 0.2)]        # over the box twice, and above everything
    grasp[:, 3:6] = [(0.0, 1.0, 0.0), (0.05, 1.0, 0.0), (0.0, 1.0, 0.0)]
    grasp[:, 6] = -np.pi / 2                                                       # approach straight down
    params = approach.ApproachParams(standoff=0.02, friction_deg=30.0, min_contact=0.5)
    res = approach.analyse_volume(vol, _dev(grasp), DEPTH, WIDTH, params, surface=surface, to_volume=np.eye(4))
    assert res.frame[0, 2, 0].item() < -0.999
    want = cloud_ref.approach_ref(surface.xyz.cpu().numpy(), surface.normal.cpu().numpy(), res.T.cpu().numpy(), GRIPPER, 0.02,
                                  params.contact_depth, cloud_ref.cos_friction(30.0))
    got = res.contact_counts.cpu().numpy()
    assert np.array_equal(got, want[0])
    assert (got[:2, 3] > 0).all() and (got[:2, 5] > 0).all() and (got[:2, 4] > 0).all() and not got[2, 3:].any()
    # T is the inverse of L: T L = identity up to the two roundings
    L4 = np.concatenate([res.L.cpu().numpy().reshape(3, 3, 4).astype(np.float64), np.tile([[[0, 0, 0, 1.0]]], (3, 1, 1))], axis=1)
    assert np.abs(res.T.cpu().numpy().astype(np.float64) @ L4 - np.eye(4)).max() < 1e-6
    kernel = (res.counts.cpu().numpy(), res.values.cpu().numpy())
    derived = ref.derived_ref(kernel[0], kernel[1], res.frame.cpu().numpy(), res.center.cpu().numpy(), params.pad, GRIPPER[4], "free", got)
    assert res.contact.cpu().numpy().tobytes() == derived["grasp_contact"].tobytes() and (derived["grasp_contact"][:2] > 0).all()
    assert np.array_equal(res.passes().cpu().numpy(), ref.passes_ref(derived, None, 0.5))
    # without a surface, or without friction_deg, the contact is 0 and nothing is estimated
    for kw, surf in (({"friction_deg": 30.0}, None), ({}, surface)):
        off = approach.analyse_volume(vol, _dev(grasp), DEPTH, WIDTH, dict(standoff=0.02, **kw), surface=surf)
        assert off.contact_counts is None and off.contact.tolist() == [0.0] * 3 and torch.equal(off.counts, res.counts)
