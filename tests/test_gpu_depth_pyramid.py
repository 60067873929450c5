"""The two image kernels of csrc/depth.hip (``depth_frame.smooth``, ``depth_frame.halve``) and the hand-over of the registration's
state block (``registration.continue_state``) on the device against the numpy restatement (tests/depth_pyramid_reference.py):
every output as uint32 bit patterns or integers, exactly; sentinel-guarded outputs, a side stream, a replayed graph, and every
error code."""
import numpy as np
import pytest
import torch

from . import depth_pyramid_reference as pyr
from . import icp_projective_reference as pref
from . import icp_reference as iref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
f32 = np.float32
SIZES = ((1, 1), (67, 3), (48, 36), (130, 70))            # (W, H): one pixel; a partial tile in both directions; whole tiles and
#                                                           a partial row of them; more than one tile either way with remainders
SENTINEL = 1234.5


def gpu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def bits(a):
    a = a.cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def image(width, height, seed=0):
    """A noisy slanted surface with a 5 cm step, and every kind of "no depth": NaN, inf, 0, negative; holes at the corners of the
    32 x 8 tiles and of the image, on its borders, and a 3 x 3 one."""
    rng = np.random.RandomState(seed + 17 * width + height)
    u, v = np.meshgrid(np.arange(width), np.arange(height))
    z = 0.6 + 0.0007 * u + 0.0004 * v + 0.002 * rng.standard_normal((height, width))
    z[:, width // 2:] += 0.05
    z = z.astype(np.float32)
    bad = (np.nan, np.inf, 0.0, -0.7, -np.inf)
    if width * height > 1:
        holes = rng.rand(height, width) < 0.06
        z[holes] = np.array(bad, dtype=np.float32)[rng.randint(0, len(bad), size=int(holes.sum()))]
        for j, (x, y) in enumerate(((31, 7), (32, 8), (32, 7), (31, 8), (0, 0), (width - 1, height - 1), (width - 1, 0), (63, 15), (64, 16))):
            if x < width and y < height:
                z[y, x] = bad[j % len(bad)]
        if width > 12 and height > 12:
            z[9:12, 9:12] = np.nan
    return z


def guarded(height, width, pad=300):
    """An (H, W) view in the middle of a sentinel-filled buffer -> (buffer, view)."""
    buf = torch.full((2 * pad + height * width,), SENTINEL, dtype=torch.float32, device=DEV)
    return buf, buf[pad:pad + height * width].view(height, width)


def guards_intact(buf, n, pad=300):
    return bool((buf[:pad] == SENTINEL).all()) and bool((buf[pad + n:] == SENTINEL).all())


# ---- smooth -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("radius", [1, 2, 3, 4])
@pytest.mark.parametrize("size", SIZES)
def test_smooth_bit_for_bit(size, radius):
    from regnet_for_3d_grasping_amd import depth_frame
    width, height = size
    z = image(width, height, radius)
    params = depth_frame.SmoothParams(radius=radius, sigma_space=1.7, sigma_depth=0.008)
    want = pyr.smooth(z, radius, 1.7, 0.008)
    buf, out = guarded(height, width)
    got = depth_frame.smooth(gpu(z), params, out=out)
    assert got is out and np.array_equal(bits(got), bits(want)) and guards_intact(buf, width * height)
    valid = pyr.has_depth(z)
    assert np.array_equal(np.isnan(want), ~valid) and (bits(want)[~valid] == 0x7FC00000).all()
    if width * height > 100:
        assert (bits(want)[valid] != bits(z)[valid]).mean() > 0.9          # (the filter did something)


def test_smooth_tables_and_the_edges_of_the_range_table():
    """``smooth_tables`` is the restatement's, bit for bit.  sigma_depth = 1 / 96 makes rbin = 8192 exactly, so t = |d| 8192 is
    exact: a neighbour 1 / 32 m behind the centre has t = 256 and is skipped, one ulp nearer has t < 256 and counts with G[255],
    one ulp further is skipped."""
    from regnet_for_3d_grasping_amd import depth_frame
    for kw in (dict(), dict(radius=1, sigma_space=0.8, sigma_depth=0.003), dict(radius=4, sigma_space=3.1, sigma_depth=0.02)):
        S, G, rbin = pyr.tables(**dict(pyr.SMOOTH_DEFAULTS, **kw))
        p = depth_frame.SmoothParams(**kw)
        assert np.array_equal(bits(depth_frame.smooth_tables(p)), bits(np.concatenate([S.reshape(-1), G])))
        assert f32(p.rbin()) == rbin
    p = depth_frame.SmoothParams(radius=1, sigma_space=1.0, sigma_depth=1.0 / 96.0)
    assert f32(p.rbin()) == f32(8192.0)
    edge = f32(0.53125)
    results = []
    for zq in (np.nextafter(edge, f32(0)), edge, np.nextafter(edge, f32(1))):
        z = np.full((3, 3), np.nan, dtype=np.float32)
        z[1, 1], z[1, 2] = f32(0.5), zq
        t = np.abs(zq - f32(0.5)) * f32(8192.0)
        got = depth_frame.smooth(gpu(z), p)
        assert np.array_equal(bits(got), bits(pyr.smooth(z, 1, 1.0, 1.0 / 96.0)))
        results.append((float(t), float(got[1, 1]), float(got[1, 2])))
    assert results[0][0] < 256.0 == results[1][0] < results[2][0]
    assert results[0][1] > 0.5 and results[1][1] == 0.5 and results[2][1] == 0.5      # counted just inside; skipped at 256 and beyond
    assert results[1][2] == float(edge)


def test_smooth_of_nothing_on_a_side_stream_and_replayed():
    from regnet_for_3d_grasping_amd import depth_frame
    for bad in (np.nan, 0.0, -1.0, np.inf):
        got = depth_frame.smooth(gpu(np.full((9, 40), bad, dtype=np.float32)))
        assert (bits(got) == 0x7FC00000).all()
    width, height = 130, 70
    z, params = image(width, height, 5), depth_frame.SmoothParams()
    want = pyr.smooth(z)
    side = torch.cuda.Stream(device=DEV)
    src = gpu(z)
    torch.cuda.synchronize()
    got = depth_frame.smooth(src, params, stream=side)
    side.synchronize()
    assert np.array_equal(bits(got), bits(want))
    # captured with static buffers (tables and out given: no upload, no allocation), replayed on new contents
    tables = gpu(depth_frame.smooth_tables(params))
    buf, out = guarded(height, width)
    torch.cuda.synchronize()
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        depth_frame.smooth(src, params, out=out, tables=tables)
    torch.cuda.current_stream(DEV).wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        depth_frame.smooth(src, params, out=out, tables=tables)
    for other in (z, np.ascontiguousarray(z[::-1]), z):
        out.fill_(9.0)
        src.copy_(gpu(other))
        graph.replay()
        torch.cuda.synchronize()
        assert np.array_equal(bits(out), bits(pyr.smooth(other))) and guards_intact(buf, width * height)


# ---- halve --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", [(67, 3), (2, 2), (48, 36), (131, 71)])
def test_halve_bit_for_bit(size):
    from regnet_for_3d_grasping_amd import depth_frame
    width, height = size
    z = image(width, height, 2)
    for cutoff in (0.02, 0.001):
        want = pyr.halve(z, cutoff)
        assert want.shape == (height // 2, width // 2)
        buf, out = guarded(height // 2, width // 2)
        got = depth_frame.halve(gpu(z), cutoff, out=out)
        assert np.array_equal(bits(got), bits(want)) and guards_intact(buf, want.size)


def test_halve_blocks_cutoff_and_ties():
    """One image of 2 x 2 blocks: every count of valid pixels with every kind of "no depth", the valid ones in every position;
    the cutoff met exactly, one ulp beyond, and a cutoff one ulp short; two and four pixels tied for the smallest."""
    from regnet_for_3d_grasping_amd import depth_frame
    nan = np.nan
    ref, cut = f32(0.5), f32(0.0078125)
    far = f32(ref + cut)
    beyond = np.nextafter(far, f32(1))
    blocks = []
    for mask in range(16):
        for bad in (nan, 0.0, -3.0, np.inf):
            blocks.append([f32(0.5 + 0.001 * k) if mask >> k & 1 else bad for k in range(4)])
    blocks += [[ref, far, nan, nan], [ref, beyond, nan, nan], [far, nan, nan, ref], [beyond, ref, far, nan],
               [ref, ref, far, beyond], [ref, ref, ref, ref], [far, ref, ref, nan], [0.7, 0.5, 0.7, 0.5]]
    z = np.array(blocks, dtype=np.float32).reshape(len(blocks), 2, 2).transpose(1, 0, 2).reshape(2, 2 * len(blocks))
    for cutoff in (cut, np.nextafter(cut, f32(0)), np.nextafter(cut, f32(1))):
        want = pyr.halve(z, cutoff)
        got = depth_frame.halve(gpu(z), float(cutoff))
        assert np.array_equal(bits(got), bits(want))
    want = pyr.halve(z, cut)[0]
    assert want[64] == (ref + far) / f32(2) and want[65] == ref and want[66] == (far + ref) / f32(2)
    assert (bits(want[:4]) == 0x7FC00000).all() and want[69] == ref


def test_halve_on_a_side_stream_and_replayed():
    from regnet_for_3d_grasping_amd import depth_frame
    width, height = 131, 71
    z = image(width, height, 8)
    src = gpu(z)
    side = torch.cuda.Stream(device=DEV)
    torch.cuda.synchronize()
    got = depth_frame.halve(src, 0.02, stream=side)
    side.synchronize()
    assert np.array_equal(bits(got), bits(pyr.halve(z, 0.02)))
    buf, out = guarded(height // 2, width // 2)
    torch.cuda.synchronize()
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        depth_frame.halve(src, 0.02, out=out)
    torch.cuda.current_stream(DEV).wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        depth_frame.halve(src, 0.02, out=out)
    for other in (z, np.ascontiguousarray(z[:, ::-1]), z):
        out.fill_(9.0)
        src.copy_(gpu(other))
        graph.replay()
        torch.cuda.synchronize()
        assert np.array_equal(bits(out), bits(pyr.halve(other, 0.02))) and guards_intact(buf, out.numel())


def test_the_pyramid_and_its_intrinsics():
    from regnet_for_3d_grasping_amd import depth_frame
    z, k = image(130, 70, 4), (150.3, 149.1, 64.2, 35.7)
    want = pyr.pyramid(z, k, 3, 0.03, dict(radius=2))
    got = depth_frame.pyramid(gpu(z), k, 3, 0.03, {"radius": 2})
    assert [(w, h) for _, _, w, h in got] == [(130, 70), (65, 35), (32, 17)] == [(w, h) for _, _, w, h in want]
    for (d, kd, _, _), (r, kr, _, _) in zip(got, want):
        assert np.array_equal(bits(d), bits(r)) and kd.astuple() == kr
    assert depth_frame.level_intrinsics(k).astuple() == pyr.level_intrinsics(k)
    plain = depth_frame.pyramid(gpu(z), k, 1, 0.03)
    assert len(plain) == 1 and np.array_equal(bits(plain[0][0]), bits(z))
    with pytest.raises(ValueError, match="levels"):
        depth_frame.pyramid(gpu(z[:3, :3]), k, 3, 0.03)


# ---- the hand-over ------------------------------------------------------------------------------------------------------------
def block(iteration, status, max_iter):
    from regnet_for_3d_grasping_amd import registration
    raw = registration.initial_state(iref.perturbation(1.0, 3.0), {"iterations": 20})
    raw[96:108].view(np.int32)[:] = (iteration, status, max_iter)
    raw[128:].view(np.float64)[:] = np.arange(128) + 0.25          # a history that must stay
    return raw


@pytest.mark.parametrize("status", range(5))
def test_continue_state_from_every_status(status):
    from regnet_for_3d_grasping_amd import registration
    for iteration, max_iter, budget in ((7, 9, 5), (60, 60, 10), (63, 64, 64), (0, 1, 1)):
        raw = block(iteration, status, max_iter)
        mark_want, status_want, max_want = pyr.continue_state(iteration, status, max_iter, budget)
        want = raw.copy()
        want[100:108].view(np.int32)[:] = (status_want, max_want)
        for with_mark in (True, False):
            state = gpu(raw)
            marks = torch.full((3, 2), -9, dtype=torch.int32, device=DEV)
            registration.continue_state(state, budget, marks[1] if with_mark else None)
            assert state.cpu().numpy().tobytes() == want.tobytes()
            assert marks.cpu().numpy().tolist() == [[-9, -9], list(mark_want) if with_mark else [-9, -9], [-9, -9]]
    if status in (iref.CONVERGED, iref.MAX_ITER):
        assert max_want == 1 and status_want == iref.RUNNING and pyr.continue_state(60, status, 60, 10)[2] == 64      # the clamp


def test_steps_after_the_hand_over():
    """A registration that CONVERGED runs on after the hand-over -- the next step counts, writes its history row and ends
    MAX_ITER at the new limit -- and one that ended TOO_FEW stays ended: the hand-over and the steps after it write nothing.
    On a side stream and replayed as a graph the same bytes."""
    from regnet_for_3d_grasping_amd import registration
    W, H, K = 80, 60, (75.0, 75.0, 39.5, 29.5)
    scene = pref.corner_room(0.5)
    pose = pref.look_at((0.45, 0.4, 0.35), (0.05, 0.05, 0.05))
    target = pref.render(scene, W, H, K, pose)
    source = pref.render(scene, W, H, K, pose @ iref.perturbation(0.3, 4.0))
    params = {"max_dist": 0.02, "association": "projective", "iterations": 20}
    tgt = registration.prepare_projective_target(gpu(target), W, H, K, params)
    src = gpu(source)
    reg = registration.icp(src, tgt, None, params)
    assert reg.status == registration.CONVERGED and reg.iterations < 20
    done = reg.state.cpu().numpy()
    state = gpu(done)
    marks = torch.zeros((2,), dtype=torch.int32, device=DEV)
    registration.continue_state(state, 1, marks)
    registration.step(src, tgt, state, params)
    after = registration.decode_state(state.cpu().numpy())
    assert marks.cpu().numpy().tolist() == [reg.iterations, registration.CONVERGED]
    assert after["iterations"] == reg.iterations + 1 and after["status"] in (registration.MAX_ITER, registration.CONVERGED)
    assert after["history"][:-1].tobytes() == reg.result()["history"].tobytes() and after["pairs"] > 3000
    assert iref.pose_distance(after["pose"], reg.pose()) < 1e-5
    # TOO_FEW stays final
    far = np.eye(4)
    far[:3, 3] = 5.0
    lost = registration.icp(src, tgt, far, params)
    assert lost.status == registration.TOO_FEW
    before = lost.state.cpu().numpy().tobytes()
    idx = torch.full((W * H,), -9, dtype=torch.int32, device=DEV)
    registration.continue_state(lost.state, 10, marks)
    registration.step(src, tgt, lost.state, params, idx_out=idx)
    assert lost.state.cpu().numpy().tobytes() == before and bool((idx == -9).all())
    assert marks.cpu().numpy().tolist() == [1, registration.TOO_FEW]
    # a side stream, then a graph replayed on a restored block
    side = torch.cuda.Stream(device=DEV)
    state = gpu(done)
    torch.cuda.synchronize()
    registration.continue_state(state, 1, marks, stream=side)
    registration.step(src, tgt, state, params, stream=side)
    side.synchronize()
    want = state.cpu().numpy().tobytes()
    assert registration.decode_state(state.cpu().numpy())["iterations"] == reg.iterations + 1
    fresh = gpu(done)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        registration.continue_state(state, 1, marks)
        registration.step(src, tgt, state, params)
    for _ in range(2):
        state.copy_(fresh)
        marks.fill_(-9)
        graph.replay()
        torch.cuda.synchronize()
        assert state.cpu().numpy().tobytes() == want and marks.cpu().numpy().tolist() == [reg.iterations, registration.CONVERGED]


# ---- errors -------------------------------------------------------------------------------------------------------------------
def test_every_error_code_and_the_python_refusals():
    from regnet_for_3d_grasping_amd import _lib, depth_frame, registration
    L = _lib.lib
    SHAPE, NULL, UNSUPPORTED = -1, -2, -3
    stream = torch.cuda.current_stream().cuda_stream
    z = gpu(image(48, 36))
    buf, out = guarded(36, 48)
    tables = gpu(depth_frame.smooth_tables())

    def bilateral(**change):
        a = dict(depth=z.data_ptr(), W=48, H=36, radius=3, tables=tables.data_ptr(), rbin=8000.0, out=out.data_ptr())
        a.update(change)
        return L.regnet_depth_bilateral_f32(*a.values(), stream)

    def halve(**change):
        a = dict(depth=z.data_ptr(), W=48, H=36, cutoff=0.02, out=out.data_ptr())
        a.update(change)
        return L.regnet_depth_halve_f32(*a.values(), stream)

    assert bilateral() == 0 and halve() == 0
    for bad in (dict(W=0), dict(H=0), dict(W=-1), dict(radius=0), dict(radius=5), dict(radius=-1)):
        assert bilateral(**bad) == SHAPE, bad
    for bad in (dict(W=1 << 11, H=(1 << 10) + 1), dict(rbin=0.0), dict(rbin=-1.0), dict(rbin=float("nan")), dict(rbin=float("inf")),
                dict(rbin=1e60), dict(rbin=1e-60)):
        assert bilateral(**bad) == UNSUPPORTED, bad
    for name in ("depth", "tables", "out"):
        assert bilateral(**{name: None}) == NULL
    for bad in (dict(W=1), dict(H=1), dict(W=0), dict(H=-2)):
        assert halve(**bad) == SHAPE, bad
    for bad in (dict(W=1 << 11, H=(1 << 10) + 1), dict(cutoff=0.0), dict(cutoff=-1.0), dict(cutoff=float("nan")),
                dict(cutoff=float("inf")), dict(cutoff=1e60), dict(cutoff=1e-60)):
        assert halve(**bad) == UNSUPPORTED, bad
    for name in ("depth", "out"):
        assert halve(**{name: None}) == NULL
    state = gpu(block(3, iref.CONVERGED, 3))
    kept = state.cpu().numpy().tobytes()
    for budget in (0, -1, 65):
        assert L.regnet_icp_state_continue(state.data_ptr(), budget, None, stream) == SHAPE
    assert L.regnet_icp_state_continue(None, 4, None, stream) == NULL
    torch.cuda.synchronize()
    assert state.cpu().numpy().tobytes() == kept                              # a refused call launched nothing
    # Python
    for bad in (dict(radius=0), dict(radius=5), dict(radius=1.5), dict(sigma_space=0.0), dict(sigma_depth=-1.0),
                dict(sigma_depth=float("nan")), dict(sigma_depth=1e-60), dict(sigma_space=float("inf"))):
        with pytest.raises(ValueError, match="smooth"):
            depth_frame.SmoothParams(**bad)
    with pytest.raises(TypeError):
        depth_frame.SmoothParams.coerce(3)
    with pytest.raises(RuntimeError, match="CUDA"):
        depth_frame.smooth(z.cpu())
    with pytest.raises(TypeError, match="float32"):
        depth_frame.smooth(z.double())
    with pytest.raises(ValueError, match="out"):
        depth_frame.smooth(z, out=z)
    with pytest.raises(ValueError, match="out"):
        depth_frame.halve(z, 0.02, out=out)
    with pytest.raises(ValueError, match="tables"):
        depth_frame.smooth(z, {"radius": 2}, tables=tables)
    with pytest.raises(ValueError, match="cutoff"):
        depth_frame.halve(z, 0.0)
    with pytest.raises(ValueError, match="2 x 2"):
        depth_frame.halve(z[:1], 0.02)
    for budget in (0, 65, 2.5):
        with pytest.raises(ValueError, match="budget"):
            registration.continue_state(state, budget)
    with pytest.raises(ValueError, match="mark"):
        registration.continue_state(state, 3, torch.zeros((3,), dtype=torch.int32, device=DEV))
    with pytest.raises(ValueError, match="state"):
        registration.continue_state(state[:100], 3)
    with pytest.raises(RuntimeError, match="CUDA"):
        registration.continue_state(state.cpu(), 3)
    assert guards_intact(buf, 48 * 36)
