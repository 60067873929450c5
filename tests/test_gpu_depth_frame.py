"""Depth frames on the device (csrc/depth.hip, depth_frame.py) against the numpy restatement of the contract
(tests/depth_reference.py): ``xyz`` and ``rgb`` as uint32 bit patterns, ``status`` and ``counts`` as integers, all exactly; the
plumbing (streams, repeated calls, host and device inputs, no synchronisation, graph capture); and ``GraspDetector`` fed a
``DepthFrame`` against the same detector fed the reference's cloud."""
import argparse
import contextlib
import io
import math
import pickle

import numpy as np
import pytest
import torch

from . import depth_reference as ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TILE_W, TILE_H = 32, 8                     # depth_points_kernel's pixel tile
MAX_PIXELS = 1 << 21
SEED = 1234
RANGE = (0.5, 1.2)
FILTER = dict(edge_threshold=0.02, min_neighbours=2)
MODES = ("none", "aligned", "registered")


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _frame(kw):
    from regnet_for_3d_grasping_amd import depth_frame
    return depth_frame.DepthFrame(**kw)


def _device(kw, params=None, **call):
    from regnet_for_3d_grasping_amd import depth_frame
    out = depth_frame.to_cloud(_frame(kw), params, device=DEV, return_status=True, **call)
    torch.cuda.synchronize()
    return tuple(t.cpu().numpy() for t in out)


def _same(got, want):
    xyz, rgb, status, counts = got
    assert xyz.dtype == np.float32 and xyz.shape == want[0].shape and rgb.dtype == np.float32 and rgb.shape == want[1].shape
    assert status.dtype == np.uint8 and counts.dtype == np.int32 and counts.shape == (8,)
    assert np.array_equal(status, want[2])
    assert counts.tolist() == want[3].tolist()
    assert np.array_equal(_bits(xyz), _bits(want[0]))
    assert np.array_equal(_bits(rgb), _bits(want[1]))


def _check(kw, **params):
    want = ref.to_cloud(**kw, **params)
    got = _device(kw, params)
    _same(got, want)
    return got, want


def _random_frame(W, H, dtype, mode, seed):
    """A seeded scene of 16 x 16 blocks on a few depth levels with zeros, a smooth slope and 1 % far outliers; float32: also NaN,
    infinities, negatives and denormals.  The colour camera of registered mode: 1.3 x the resolution, 3 cm to the side, slightly turned."""
    rng = np.random.RandomState(seed)
    level = rng.choice([800.0, 1000.0, 1030.0, 1500.0], size=((H + 15) // 16, (W + 15) // 16))
    mm = np.kron(level, np.ones((16, 16)))[:H, :W] + 2.0 * np.arange(W)[None, :] + rng.normal(0, 1.0, (H, W))
    mm[rng.rand(H, W) < 0.01] = 9000.0
    depth = np.rint(mm).astype(np.uint16)
    depth[rng.rand(H, W) < 0.1] = 0
    if dtype == np.float32:
        depth = (depth.astype(np.float32) * np.float32(0.001)).astype(np.float32)
        kind = rng.rand(H, W)
        depth[kind < 0.02] = np.nan
        depth[(kind >= 0.02) & (kind < 0.03)] = np.inf
        depth[(kind >= 0.03) & (kind < 0.04)] = -1.0
        depth[(kind >= 0.04) & (kind < 0.05)] = -np.inf
        depth[(kind >= 0.05) & (kind < 0.07)] = 1e-41                 # a denormal: has depth, inside the default range
    f = 0.8 * max(W, 4)
    kw = {"depth": depth, "intrinsics": (f, f * 1.01, (W - 1) / 2.0, (H - 1) / 2.0), "depth_scale": 0.001}
    if mode == "aligned":
        kw["color"] = rng.randint(0, 256, size=(H, W, 3)).astype(np.uint8)
    if mode == "registered":
        Wc, Hc = max(1, int(W * 1.3)), max(1, int(H * 1.3))
        a = math.radians(2.0)
        T = np.eye(4)
        T[:3, :3] = [[math.cos(a), 0, math.sin(a)], [0, 1, 0], [-math.sin(a), 0, math.cos(a)]]
        T[:3, 3] = [-0.03, 0.002, 0.001]
        kw.update(color=rng.randint(0, 256, size=(Hc, Wc, 3)).astype(np.uint8), depth_to_color=T,
                  color_intrinsics=(1.3 * f, 1.31 * f, (Wc - 1) / 2.0 + 0.7, (Hc - 1) / 2.0 - 0.4))
    return kw


@pytest.fixture(scope="module")
def frame():
    return ref.synthetic_depth_frame()


def _mode_kw(frame, mode):
    return ref.frame_kwargs(frame, registered=mode == "registered", aligned=mode == "aligned")


# ---- sizes --------------------------------------------------------------------------------------------------------------------
SIZES = [(1, 1), (1, 7), (7, 1), (3, 3)] + [(w, h) for w in (TILE_W - 1, TILE_W, TILE_W + 1) for h in (TILE_H - 1, TILE_H, TILE_H + 1)] \
    + [(131, 67)]


@pytest.mark.parametrize("W,H", SIZES, ids=["%dx%d" % s for s in SIZES])
def test_sizes_for_both_depth_dtypes_and_all_colour_modes(W, H):
    seen = np.zeros(8, dtype=np.int64)
    for dtype in (np.uint16, np.float32):
        for mode in MODES:
            # (uint16: the 9 m outliers are out of range; float32: the default range, which keeps the denormal depths)
            extra = {"depth_range": (0.3, 5.0)} if dtype == np.uint16 else {}
            _, want = _check(_random_frame(W, H, dtype, mode, W * 100 + H), edge_threshold=0.02, min_neighbours=4, **extra)
            seen += want[3]
    print(seen.tolist())
    if (W, H) == (131, 67):
        assert (seen[[0, 1, 2, 3, 4, 6]] > 0).all()                # every status code but "occluded" (the synthetic frame's tests)


@pytest.mark.parametrize("mode", MODES)
def test_640x480_synthetic_frame(frame, mode):
    got, want = _check(_mode_kw(frame, mode), **FILTER)
    assert want[3][6] > 250000
    metres = dict(_mode_kw(frame, mode), depth=(frame.depth.astype(np.float32) * np.float32(0.001)).astype(np.float32))
    same = _device(metres, FILTER)                                 # float32 metres holding the same values: the same bytes
    _same(same, want)


@pytest.mark.parametrize("mode", MODES)
def test_largest_frame(mode):
    """2048 x 1024 = 2^21 depth pixels (registered: against the largest colour image, 4096 x 2048 = 2^23): the counts and a
    strided sample of rows."""
    W, H = 2048, 1024
    small = _random_frame(256, 128, np.uint16, "none", 77)
    kw = dict(small, depth=np.tile(small["depth"], (8, 8)), intrinsics=(1500.0, 1500.0, 1023.5, 511.5))
    rng = np.random.RandomState(3)
    params = dict(FILTER)
    if mode == "aligned":
        kw["color"] = np.tile(rng.randint(0, 256, size=(128, 256, 3)).astype(np.uint8), (8, 8, 1))
    if mode == "registered":
        T = np.eye(4)
        T[:3, 3] = [-0.03, 0.002, 0.001]
        kw.update(color=np.tile(rng.randint(0, 256, size=(256, 512, 3)).astype(np.uint8), (8, 8, 1)), depth_to_color=T,
                  color_intrinsics=(3000.0, 3000.0, 2047.5, 1023.5))
        params["splat"] = 0
    assert kw["depth"].shape == (H, W) and W * H == MAX_PIXELS
    want = ref.to_cloud(**kw, **params)
    got = _device(kw, params)
    assert got[3].tolist() == want[3].tolist()
    rows = np.r_[np.arange(0, W * H, 997), W * H - 1]
    _same(tuple(a[rows] for a in got[:3]) + (got[3],), tuple(a[rows] for a in want[:3]) + (want[3],))
    assert np.array_equal(got[2], want[2])


def test_one_pixel_over_the_limit_is_an_error_and_launches_nothing():
    from regnet_for_3d_grasping_amd import _lib, depth_frame
    W = MAX_PIXELS + 1
    depth = torch.ones((1, W), dtype=torch.float32, device=DEV)
    with pytest.raises(ValueError):
        depth_frame.to_cloud(depth_frame.DepthFrame(depth, (500.0, 500.0, 0.0, 0.0)), device=DEV)
    outs = [torch.full((64,), 7, dtype=torch.uint8, device=DEV) for _ in range(4)]
    consts = np.zeros(25, dtype=np.float32)
    torch.cuda.synchronize()
    code = _lib.lib.regnet_depth_to_cloud_f32(depth.data_ptr(), W, 1, consts.ctypes.data, None, 0, 0, 0, 0, 0, 1, 0,
                                              *(t.data_ptr() for t in outs), None, None)
    torch.cuda.synchronize()
    assert code == -3 and all(bool((t == 7).all()) for t in outs)
    color = torch.zeros((1, (1 << 23) + 1, 3), dtype=torch.uint8, device=DEV)
    code = _lib.lib.regnet_depth_to_cloud_f32(depth.data_ptr(), 8, 1, consts.ctypes.data, color.data_ptr(), (1 << 23) + 1, 1, 2, 0, 0,
                                              1, 0, *(t.data_ptr() for t in outs), outs[0].data_ptr(), None)
    torch.cuda.synchronize()
    assert code == -3 and all(bool((t == 7).all()) for t in outs)
    with pytest.raises(ValueError):
        depth_frame.to_cloud(depth_frame.DepthFrame(depth[:, :8], (5.0, 5.0, 0.0, 0.0), color=color, color_intrinsics=(5.0, 5.0, 0, 0),
                                                    depth_to_color=np.eye(4)), device=DEV)


# ---- contents -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_all_zero_and_all_65535(mode):
    base = _random_frame(70, 19, np.uint16, mode, 5)
    got, _ = _check(dict(base, depth=np.zeros((19, 70), dtype=np.uint16)), **FILTER)
    assert got[3].tolist() == [70 * 19, 0, 0, 0, 0, 0, 0, 0] and (_bits(got[0]) == ref.QNAN_BITS).all() and not got[1].any()
    full = dict(base, depth=np.full((19, 70), 65535, dtype=np.uint16))
    got, _ = _check(full, **FILTER)                                  # 65.535 m everywhere: in the default range
    assert got[3][0] == 0 and got[3][1] == 0
    got, _ = _check(full, depth_range=(0.1, 10.0), **FILTER)
    assert got[3].tolist() == [0, 70 * 19, 0, 0, 0, 0, 0, 0]
    got, _ = _check(full, depth_range=(0.1, float(np.float32(65535) * np.float32(0.001))))      # z == hi: kept
    assert got[3][1] == 0


def test_threshold_and_margin_equalities():
    K2 = (256.0, 128.0, 2.0, 1.0)
    t = 2.0 ** -6
    z = np.array([[1.0, 1.0 + t]], dtype=np.float32)
    got, _ = _check({"depth": z, "intrinsics": K2}, edge_threshold=t)
    assert got[2].tolist() == [6, 6]                                 # equality: not a jump
    z[0, 1] = np.nextafter(np.float32(1.0 + t), np.float32(2))
    got, _ = _check({"depth": z, "intrinsics": K2}, edge_threshold=t)
    assert got[2].tolist() == [2, 2]                                 # one float above: a jump, on both sides
    for k, corner in ((3, 6), (4, 3)):
        got, _ = _check({"depth": np.ones((3, 3), dtype=np.float32), "intrinsics": K2}, min_neighbours=k)
        assert got[2][0] == corner and got[2][4] == 6
    # two depth pixels on one colour pixel (a colour camera of half the horizontal resolution): the margin is inclusive
    K, Kh = (4.0, 4.0, 1.5, 0.0), (2.0, 4.0, 0.75, 0.0)
    near, far = 1.0, 1.25
    below = float(np.nextafter(np.float32(far - near), np.float32(0)))
    colour = np.arange(9, dtype=np.uint8).reshape(1, 3, 3)
    kw = {"depth": np.array([[near, far, near, far]], dtype=np.float32), "intrinsics": K, "color": colour, "color_intrinsics": Kh,
          "depth_to_color": np.eye(4)}
    got, _ = _check(kw, occlusion_margin=below, splat=0)
    assert got[2].tolist() == [6, 5, 6, 6] and (_bits(got[0][1]) == ref.QNAN_BITS).all()
    got, _ = _check(kw, occlusion_margin=below, splat=0, keep_uncoloured=True)
    assert got[2].tolist() == [6, 5, 6, 6] and got[0][1].tolist() == [-0.125 * far, 0.0, far] and not got[1][1].any()
    got, _ = _check(kw, occlusion_margin=far - near, splat=0)
    assert got[2].tolist() == [6, 6, 6, 6]
    got, _ = _check(dict(kw, depth=np.array([[near, near, near, far]], dtype=np.float32)), occlusion_margin=0.0, splat=0)
    assert got[2].tolist() == [6, 6, 6, 6]                           # equal z' on one pixel: both visible


@pytest.mark.parametrize("splat", [0, 1, 2])
@pytest.mark.parametrize("keep", [False, True], ids=["drop", "keep"])
def test_splat_and_keep_uncoloured(frame, splat, keep):
    """The synthetic frame's second camera, and the same frame seen by a colour camera of a third of the resolution, where up
    to nine depth pixels share a colour pixel."""
    kw = _mode_kw(frame, "registered")
    got, want = _check(kw, splat=splat, keep_uncoloured=keep, **FILTER)
    assert want[3][4] > 0 and want[3][5] > 0
    assert np.isfinite(got[0][got[2] == 5]).all() == keep
    coarse = dict(kw, color=np.ascontiguousarray(frame.color[::3, ::3]), color_intrinsics=tuple(c / 3.0 for c in frame.color_intrinsics))
    _check(coarse, splat=splat, keep_uncoloured=keep, occlusion_margin=0.004)


def test_colour_camera_that_sees_little(frame):
    """A colour camera turned by 60 degrees: most points are beside its image; turned right round: all are behind it."""
    a = math.radians(60.0)
    T = np.eye(4)
    T[:3, :3] = [[math.cos(a), 0, math.sin(a)], [0, 1, 0], [-math.sin(a), 0, math.cos(a)]]
    T[:3, 3] = [0.3, 0.0, 0.6]
    kw = dict(_mode_kw(frame, "registered"), depth_to_color=T)
    got, want = _check(kw, **FILTER)
    assert want[3][4] > 100000 and want[3][6] > 0
    T[:3, :3] = -np.eye(3)                                            # everything behind
    got, want = _check(dict(kw, depth_to_color=T))
    assert want[3][6] == 0 and want[3][5] == 0 and want[3][4] == int((frame.depth != 0).sum())
    T = np.eye(4)
    T[0, 3] = np.nan                                                  # NaN coordinates fail the float test
    got, want = _check(dict(kw, depth_to_color=T), keep_uncoloured=True)
    assert want[3][6] == 0 and want[3][4] == int((frame.depth != 0).sum())


# ---- plumbing -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_stream_repeat_and_device_inputs(frame, mode):
    from regnet_for_3d_grasping_amd import depth_frame
    kw = _mode_kw(frame, mode)
    want = ref.to_cloud(**kw, **FILTER)
    host = _device(kw, FILTER)
    _same(host, want)
    on_device = {key: (torch.from_numpy(value).to(DEV) if isinstance(value, np.ndarray) and key != "depth_to_color" else value)
                 for key, value in kw.items()}
    torch.cuda.synchronize()
    _same(_device(on_device, FILTER), want)                          # device-tensor inputs: the same bytes
    fr = _frame(on_device)
    first = depth_frame.to_cloud(fr, FILTER, return_status=True)
    ws = torch.empty((max(16, depth_frame.workspace_bytes(640, 480, 800, 600, 2)),), dtype=torch.uint8, device=DEV)
    out = tuple(first) + (ws,)
    for t in first:
        t.fill_(3)
    for _ in range(2):                                               # a repeated call into the same buffers
        again = depth_frame.to_cloud(fr, FILTER, return_status=True, out=out)
        assert all(a is b for a, b in zip(again, first))
        torch.cuda.synchronize()
        _same(tuple(t.cpu().numpy() for t in again), want)
    side = torch.cuda.Stream(device=DEV)
    torch.cuda.synchronize()
    got = depth_frame.to_cloud(fr, FILTER, stream=side, return_status=True)
    side.synchronize()
    _same(tuple(t.cpu().numpy() for t in got), want)


@pytest.mark.parametrize("mode", MODES)
def test_to_cloud_does_not_synchronise_and_is_capturable(frame, mode):
    from regnet_for_3d_grasping_amd import depth_frame
    kw = _mode_kw(frame, mode)
    want = ref.to_cloud(**kw, **FILTER)
    fr = _frame({key: (torch.from_numpy(value).to(DEV) if isinstance(value, np.ndarray) and key != "depth_to_color" else value)
                 for key, value in kw.items()})
    warm = depth_frame.to_cloud(fr, FILTER, return_status=True)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")                          # any blocking call is now an error
    try:
        got = depth_frame.to_cloud(fr, FILTER, return_status=True)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    _same(tuple(t.cpu().numpy() for t in got), want)
    # captured into a graph with static buffers, replayed on new contents of the same depth tensor
    ws = torch.empty((max(16, depth_frame.workspace_bytes(640, 480, 800, 600, 2)),), dtype=torch.uint8, device=DEV)
    out = tuple(warm) + (ws,)
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        depth_frame.to_cloud(fr, FILTER, return_status=True, out=out)
    torch.cuda.current_stream(DEV).wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        depth_frame.to_cloud(fr, FILTER, return_status=True, out=out)
    flipped = np.ascontiguousarray(frame.depth[::-1])
    for depth in (frame.depth, flipped, frame.depth):
        for t in warm:
            t.fill_(9)
        fr.depth.copy_(torch.from_numpy(depth).to(DEV))
        graph.replay()
        torch.cuda.synchronize()
        _same(tuple(t.cpu().numpy() for t in warm), ref.to_cloud(**dict(kw, depth=depth), **FILTER))


# ---- the detector -------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def detector_parts(frame):
    """Networks calibrated on the depth frame's own cropped cloud (the recipe of tests/test_gpu_table_plane.py); the cloud is
    the REFERENCE's, for the registered colour camera with the filter on."""
    from regnet_for_3d_grasping_amd import depth_frame, detect, np_random, pipeline, synthetic
    from regnet_for_3d_grasping_amd.get_regiondataset import get_grasp_allobj
    from . import test_gpu_detect as td
    kw = _mode_kw(frame, "registered")
    xyz, rgb = ref.to_cloud(**kw, **FILTER)[:2]
    score_net, region_net = pipeline.build_models(DEV)
    score_net.eval()
    region_net.eval()
    probe = detect.GraspDetector(score_net, region_net)
    np.random.seed(SEED)
    with np_random.deferred(), torch.no_grad():
        pc = probe.ingest((xyz, rgb)).pc.clone()
    synthetic.calibrate_score_head(score_net, pc)
    with torch.no_grad():
        feat, score, _ = score_net(pc)
    np.random.seed(41)
    got = get_grasp_allobj(pc, score, detect.TEST_PARAMS, [], True)
    np.random.seed(5)
    synthetic.calibrate_region_head(region_net, lambda: td._region(region_net, got, pc, feat, detect.GRIPPER_PARAMS))
    return score_net, region_net, (xyz, rgb), depth_frame.DepthFrame(**kw)


def _run(parts, source, **kw):
    from regnet_for_3d_grasping_amd import detect
    detector = detect.GraspDetector(parts[0], parts[1], **kw)
    np.random.seed(SEED)
    out = detector.detect(source)
    return out, np.random.get_state()


def _same_state(a, b):
    return a[0] == b[0] and np.array_equal(a[1], b[1]) and a[2:] == b[2:]


def test_detect_of_a_depth_frame_equals_detect_of_the_reference_cloud(detector_parts):
    from regnet_for_3d_grasping_amd import detect
    got, got_state = _run(detector_parts, detector_parts[3], depth=FILTER)
    want, want_state = _run(detector_parts, detector_parts[2])
    assert tuple(got) == tuple(want) == detect.RESULT_KEYS
    assert len(want["points"]) > 20000
    print("depth frame: %d points kept, %d / %d / %d grasps" % (len(got["points"]), len(got["grasp_stage2"]),
                                                                len(got["grasp_stage3"]), len(got["grasp_stage3_score"])))
    for key in detect.RESULT_KEYS:
        assert got[key].dtype == want[key].dtype and got[key].tobytes() == want[key].tobytes(), key
    assert _same_state(got_state, want_state)
    # a detector built without `depth` gives the bytes it gave before on a .pcd-style pair
    plain, _ = _run(detector_parts, detector_parts[2], depth=None)
    other, _ = _run(detector_parts, detector_parts[2], depth={"edge_threshold": 0.5, "min_neighbours": 8})
    for key in detect.RESULT_KEYS:
        assert plain[key].tobytes() == want[key].tobytes() == other[key].tobytes(), key


def test_detect_of_a_depth_frame_with_the_table_estimated(detector_parts):
    """Both detectors estimate the table on byte-identical clouds (the test above), each with an estimate of its own: the
    refit's moments are summed in a fixed order (``table_plane.moments_fixed_order``), so the two transforms are the same bits."""
    from regnet_for_3d_grasping_amd import detect
    got, _ = _run(detector_parts, detector_parts[3], depth=FILTER, transform={"range": RANGE})
    want, _ = _run(detector_parts, detector_parts[2], transform={"range": RANGE})
    assert tuple(got) == tuple(want) == detect.RESULT_KEYS + detect.TABLE_KEYS
    for key in detect.TABLE_KEYS:
        assert got[key].tobytes() == want[key].tobytes(), key
    for key in detect.RESULT_KEYS:
        assert got[key].dtype == want[key].dtype and got[key].tobytes() == want[key].tobytes(), key


def test_detect_of_a_depth_frame_with_the_first_estimate_given(detector_parts):
    """The depth frame with the table estimated per frame against the reference's cloud with THAT estimate given explicitly:
    byte for byte (what tests/test_gpu_table_plane.py does for a cloud)."""
    from regnet_for_3d_grasping_amd import detect
    got, state = _run(detector_parts, detector_parts[3], depth=FILTER, transform={"range": RANGE})
    want, want_state = _run(detector_parts, detector_parts[2], transform=got["table_transform"])
    assert tuple(want) == detect.RESULT_KEYS
    for key in detect.RESULT_KEYS:
        assert got[key].dtype == want[key].dtype and got[key].tobytes() == want[key].tobytes(), key
    assert _same_state(state, want_state)


def test_cli_on_a_folder_with_one_npz(detector_parts, tmp_path):
    import glob
    from regnet_for_3d_grasping_amd import depth_frame, detect
    folder = tmp_path / "real_data"
    folder.mkdir()
    path = str(folder / "frame.npz")
    depth_frame.save_npz(path, detector_parts[3])
    assert glob.glob(str(folder) + "/*.npz") == [path]
    flags = argparse.Namespace(depth_range=None, edge_threshold=FILTER["edge_threshold"], min_neighbours=FILTER["min_neighbours"],
                               occlusion_margin=None, keep_uncoloured=False)
    detector = detect.GraspDetector(detector_parts[0], detector_parts[1], depth=detect.depth_from_args(flags))
    np.random.seed(SEED)
    printed = io.StringIO()
    with contextlib.redirect_stdout(printed):
        out, saved = detector.detect_file(path, real_data=True)
    assert saved == str(tmp_path / "real_data_predict" / "frame.p") and len(printed.getvalue().strip().splitlines()) == 3
    with open(saved, "rb") as f:
        record = pickle.load(f)
    assert tuple(record) == detect.RESULT_KEYS
    want, _ = _run(detector_parts, detector_parts[2])
    for key in detect.RESULT_KEYS:
        assert record[key].tobytes() == want[key].tobytes(), key
