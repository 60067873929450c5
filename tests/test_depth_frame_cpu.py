"""Depth frames without a GPU: the C ABI's new entry points (exported, declared, argument checks before any launch, the
workspace formula at its limits), the numpy restatement of the contract (tests/depth_reference.py) against answers derived by
hand, the filter's and the occlusion test's measured effect on the synthetic depth frame, and ``detect``'s helpers."""
import argparse
import ctypes
import os
import re

import numpy as np
import pytest

from . import depth_reference as ref

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("regnet_depth_workspace_bytes", "regnet_depth_colour_lut", "regnet_depth_to_cloud_u16", "regnet_depth_to_cloud_f32")
MAX_PIXELS, MAX_COLOUR = 1 << 21, 1 << 23
f32 = np.float32
K2 = (256.0, 128.0, 2.0, 1.0)             # power-of-two intrinsics: every product below is exact


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ---- ABI and arguments ------------------------------------------------------------------------------------------------------
def test_new_symbols_are_exported_bound_and_declared():
    from regnet_for_3d_grasping_amd import _lib, depth_frame
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "regnet_hip.h")).read(), flags=re.S)
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert hasattr(raw, name), name
        assert name in _lib.SIGNATURES, name
        assert re.search(r"\b%s\s*\(" % name, header), name
    assert len(_lib.SIGNATURES["regnet_depth_to_cloud_u16"][1]) == 18 == len(_lib.SIGNATURES["regnet_depth_to_cloud_f32"][1])
    assert _lib.HAS_STREAM["regnet_depth_to_cloud_u16"] and not _lib.HAS_STREAM["regnet_depth_workspace_bytes"]
    assert _lib.lib.regnet_abi_version() == 2
    assert depth_frame.MAX_DEPTH_PIXELS == MAX_PIXELS and depth_frame.MAX_COLOR_PIXELS == MAX_COLOUR


@pytest.mark.parametrize("name", NEW_SYMBOLS[2:])
def test_argument_checks_without_gpu(name):
    from regnet_for_3d_grasping_amd import _lib
    fn = getattr(_lib.lib, name)
    params = np.zeros(25, dtype=np.float32)

    def call(W, H, Wc=0, Hc=0, mode=0, k=0, r=1, ptr=1, colour=1, ws=1, par=True):
        # validation happens before any launch, so these are safe without a device
        return fn(ptr, W, H, params.ctypes.data if par else None, colour, Wc, Hc, mode, 1, k, r, 0, ptr, ptr, ptr, ptr, ws, None)
    for W, H in ((0, 4), (4, 0), (-1, 4), (4, -1)):
        assert call(W, H) == -1
    assert call(4, 4, mode=3) == -1 and call(4, 4, mode=-1) == -1
    assert call(4, 4, k=9) == -1 and call(4, 4, k=-1) == -1 and call(4, 4, r=3) == -1 and call(4, 4, r=-1) == -1
    assert call(4, 4, 4, 5, mode=1) == -1 and call(4, 4, 5, 4, mode=1) == -1          # aligned: the depth grid
    assert call(4, 4, 0, 8, mode=2) == -1 and call(4, 4, 8, 0, mode=2) == -1
    assert call(MAX_PIXELS + 1, 1) == -3 and call(1, MAX_PIXELS + 1) == -3 and call(2049, 1024) == -3
    assert call(1 << 40, 1 << 40) == -3
    assert call(4, 4, MAX_COLOUR + 1, 1, mode=2) == -3 and call(4, 4, 4097, 2048, mode=2) == -3
    assert call(4, 4, ptr=None) == -2 and call(4, 4, par=False) == -2
    assert call(4, 4, 4, 4, mode=1, colour=None) == -2 and call(4, 4, 8, 8, mode=2, colour=None) == -2
    assert call(4, 4, 8, 8, mode=2, ws=None) == -2
    # the limits themselves are supported (the null pointer is found after them); k and r at their ends
    assert call(MAX_PIXELS, 1, ptr=None) == -2 and call(2048, 1024, 4096, 2048, mode=2, k=8, r=2, ptr=None) == -2
    assert call(1920, 1080, 1920, 1080, mode=1, r=0, ptr=None) == -2


def test_workspace_size_formula():
    from regnet_for_3d_grasping_amd import _lib, depth_frame
    ws = _lib.lib.regnet_depth_workspace_bytes
    for W, H in ((1, 1), (640, 480), (1920, 1080), (MAX_PIXELS, 1), (1, MAX_PIXELS), (2048, 1024)):
        assert ws(W, H, 0, 0, 0) == 16 and ws(W, H, W, H, 1) == 16 == depth_frame.workspace_bytes(W, H, W, H, 1)
        for Wc, Hc in ((1, 1), (3, 1), (5, 1), (800, 600), (MAX_COLOUR, 1), (1, MAX_COLOUR), (4096, 2048)):
            want = (4 * Wc * Hc + 15) // 16 * 16
            assert ws(W, H, Wc, Hc, 2) == want == depth_frame.workspace_bytes(W, H, Wc, Hc, 2)
    assert ws(1, 1, 1, 1, 2) == 16 and ws(1, 1, 5, 1, 2) == 32
    for args in ((0, 1, 0, 0, 0), (1, 0, 0, 0, 0), (MAX_PIXELS + 1, 1, 0, 0, 0), (2049, 1024, 0, 0, 0), (4, 4, 0, 0, 3),
                 (4, 4, 4, 5, 1), (4, 4, 0, 1, 2), (4, 4, MAX_COLOUR + 1, 1, 2), (4, 4, 4097, 2048, 2), (4, 4, 1, MAX_COLOUR + 1, 2)):
        assert ws(*args) == -1, args


def test_lut():
    from regnet_for_3d_grasping_amd import depth_frame
    lut = ref.lut()
    assert lut.dtype == np.float32 and lut[0] == 0 and lut[255] == 1 and (np.diff(lut) > 0).all()
    assert lut[51] == f32(0.2) and lut[1] == f32(1.0 / 255.0)
    assert _bits(depth_frame.colour_lut()).tolist() == _bits(lut).tolist()          # the table in the library


# ---- the reference against answers derived by hand ----------------------------------------------------------------------------
def test_deprojection_with_power_of_two_intrinsics():
    depth = np.array([[1024, 2048, 512, 0, 4096], [256, 1024, 1024, 8192, 64]], dtype=np.uint16)
    xyz, rgb, status, counts = ref.to_cloud(depth, K2, depth_scale=2.0 ** -10)
    z = depth.astype(np.float64) / 1024.0
    u, v = np.meshgrid(np.arange(5.0), np.arange(2.0))
    want = np.stack([(u - 2.0) * z / 256.0, (v - 1.0) * z / 128.0, z], axis=-1).reshape(-1, 3)
    kept = depth.reshape(-1) != 0
    assert np.array_equal(xyz[kept].astype(np.float64), want[kept])                  # exact: no rounding anywhere
    assert _bits(xyz[~kept]).tolist() == [[ref.QNAN_BITS] * 3]
    assert status.tolist() == [6, 6, 6, 0, 6, 6, 6, 6, 6, 6] and counts.tolist() == [1, 0, 0, 0, 0, 0, 9, 0]
    assert not rgb.any() and xyz.dtype == rgb.dtype == np.float32 and status.dtype == np.uint8 and counts.dtype == np.int32
    # float32 metres: the same cloud; a NaN, an infinity, a negative and a zero are "no depth"
    metres = (depth.astype(np.float32) / f32(1024)).astype(np.float32)
    again = ref.to_cloud(metres, K2)
    assert _bits(again[0]).tolist() == _bits(xyz).tolist() and again[2].tolist() == status.tolist()
    metres[0, :4] = [np.nan, np.inf, -1.0, 0.0]
    assert ref.to_cloud(metres, K2)[2].tolist() == [0, 0, 0, 0, 6, 6, 6, 6, 6, 6]


def test_range_is_inclusive():
    depth = np.array([[499, 500, 501, 1999, 2000, 2001, 0]], dtype=np.uint16)
    lo, hi = float(f32(500) * f32(0.001)), float(f32(2000) * f32(0.001))
    assert ref.to_cloud(depth, K2, depth_range=(lo, hi))[2].tolist() == [1, 6, 6, 6, 6, 1, 0]
    z = np.array([[0.25, 0.5, 0.75, 1.0, 1.5]], dtype=np.float32)
    assert ref.to_cloud(z, K2, depth_range=(0.5, 1.0))[2].tolist() == [1, 6, 6, 6, 1]


def test_jump_exactly_at_the_threshold():
    t = 2.0 ** -6
    z = np.array([[1.0, 1.0 + t]], dtype=np.float32)               # |z - zq| = 2^-6 = t * min: not a jump at equality
    assert ref.to_cloud(z, K2, edge_threshold=t)[2].tolist() == [6, 6]
    z[0, 1] = np.nextafter(f32(1.0 + t), f32(2))                   # one float above
    assert ref.to_cloud(z, K2, edge_threshold=t)[2].tolist() == [2, 2]          # symmetric: both sides lose a pixel
    assert ref.to_cloud(z, K2, edge_threshold=None)[2].tolist() == [6, 6]
    # decided on valid0 only, in one pass: the middle pixel is out of range, so its neighbours do not see it
    z = np.array([[1.0, 3.0, 1.0]], dtype=np.float32)
    assert ref.to_cloud(z, K2, edge_threshold=t, depth_range=(0.0, 2.0))[2].tolist() == [6, 1, 6]
    # a removed pixel still removes: a staircase 1, 1.1, 1.2 goes whole
    z = np.array([[1.0, 1.1, 1.2]], dtype=np.float32)
    assert ref.to_cloud(z, K2, edge_threshold=t)[2].tolist() == [2, 2, 2]
    # diagonal neighbours count
    z = np.array([[1.0, 1.0], [1.0, 2.0]], dtype=np.float32)
    assert ref.to_cloud(z, K2, edge_threshold=t)[2].tolist() == [2, 2, 2, 2]


def test_borders_and_min_neighbours():
    one = np.ones((3, 3), dtype=np.float32)
    for k, want in ((3, [6] * 9), (4, [3, 6, 3, 6, 6, 6, 3, 6, 3]), (6, [3, 3, 3, 3, 6, 3, 3, 3, 3]), (8, [3] * 4 + [6] + [3] * 4)):
        # a corner has 3 neighbours inside the image, an edge pixel 5: beyond the border is neither a jump nor a neighbour
        assert ref.to_cloud(one, K2, edge_threshold=0.01, min_neighbours=k)[2].tolist() == want, k
    lone = np.zeros((3, 3), dtype=np.float32)
    lone[1, 1] = 1.0
    assert ref.to_cloud(lone, K2, min_neighbours=0)[2].tolist() == [0] * 4 + [6] + [0] * 4
    assert ref.to_cloud(lone, K2, min_neighbours=1)[2].tolist() == [0] * 4 + [3] + [0] * 4
    assert ref.to_cloud(np.ones((1, 1), dtype=np.float32), K2, edge_threshold=0.01)[2].tolist() == [6]
    # an out-of-range neighbour is no neighbour
    z = np.array([[1.0, 5.0, 1.0]], dtype=np.float32)
    assert ref.to_cloud(z, K2, depth_range=(0, 2), min_neighbours=1)[2].tolist() == [3, 1, 3]


def test_status_precedence():
    # no depth < out of range < edge jump < too few neighbours < outside < occluded
    z = np.array([[0.0, 9.0, 1.0, 2.0]], dtype=np.float32)
    kw = dict(depth_range=(0.0, 5.0), edge_threshold=0.01, min_neighbours=8)
    xyz, rgb, status, counts = ref.to_cloud(z, K2, **kw)
    assert status.tolist() == [0, 1, 2, 2] and counts.tolist() == [1, 1, 2, 0, 0, 0, 0, 0]      # a jump before the count
    assert ref.to_cloud(z, K2, depth_range=(0.0, 5.0), min_neighbours=8)[2].tolist() == [0, 1, 3, 3]
    assert (_bits(xyz) == ref.QNAN_BITS).all() and not rgb.any()
    # a filtered pixel takes no part in the colour camera's z-buffer: it cannot occlude
    colour = np.full((1, 4, 3), 255, dtype=np.uint8)
    reg = dict(color=colour, color_intrinsics=K2, depth_to_color=np.eye(4))
    assert ref.to_cloud(z, K2, **kw, **reg)[2].tolist() == [0, 1, 2, 2]


def test_occlusion_at_the_margin():
    """Two fronto-parallel planes (depth 1 and 1.25, alternating pixels of one row) seen by a colour camera of half the
    horizontal resolution: a near and a far point land on colour pixel 1."""
    K = (4.0, 4.0, 1.5, 0.0)
    near, far = 1.0, 1.25
    gap = far - near
    below = float(np.nextafter(f32(gap), f32(0)))
    Kh = (2.0, 4.0, 0.75, 0.0)
    T = np.eye(4)
    zz = np.array([[near, far, near, far]], dtype=np.float32)
    # uc = (u - 1.5) / 4 * 2 + 0.75 = u / 2: 0, 0.5, 1, 1.5 -> fu = floor(uc + 0.5) = 0, 1, 1, 2
    colour = np.arange(3 * 3, dtype=np.uint8).reshape(1, 3, 3)
    kw = dict(color=colour, color_intrinsics=Kh, depth_to_color=T, splat=0, details=True)
    xyz, rgb, status, counts, ex = ref.to_cloud(zz, K, occlusion_margin=below, **kw)
    assert ex.fu.reshape(-1).tolist() == [0, 1, 1, 2] and ex.inside.all()
    assert status.tolist() == [6, 5, 6, 6]                          # the far point on pixel 1 is occluded by the near one
    assert ex.zbuffer.reshape(-1).tolist() == [near, near, far]
    xyz, rgb, status, counts, ex = ref.to_cloud(zz, K, occlusion_margin=gap, **kw)
    assert status.tolist() == [6, 6, 6, 6]                          # z' - zmin = margin: visible (inclusive)
    assert _bits(rgb[1]).tolist() == _bits(ref.lut()[colour[0, 1]]).tolist()
    # equal z' on one pixel: both visible, at margin 0
    same = np.array([[near, near, near, far]], dtype=np.float32)
    assert ref.to_cloud(same, K, occlusion_margin=0.0, **kw)[2].tolist() == [6, 6, 6, 6]
    # dropped or kept without colour
    xyz, rgb, status, _, _ = ref.to_cloud(zz, K, occlusion_margin=below, **kw)
    assert (_bits(xyz[1]) == ref.QNAN_BITS).all() and not rgb[1].any()
    kw["keep_uncoloured"] = True
    xyz, rgb, status, _, _ = ref.to_cloud(zz, K, occlusion_margin=below, **kw)
    assert status.tolist() == [6, 5, 6, 6] and xyz[1].tolist() == [-0.125 * far, 0.0, far] and not rgb[1].any()


def test_footprint_is_clipped_at_the_border_and_widens_the_occluder():
    K = (4.0, 4.0, 1.5, 0.0)
    z = np.array([[1.0, 2.0, 2.0, 2.0]], dtype=np.float32)
    colour = np.zeros((1, 4, 3), dtype=np.uint8)
    kw = dict(color=colour, color_intrinsics=K, depth_to_color=np.eye(4), occlusion_margin=0.5, details=True)
    for r, want_zb, want in ((0, [1, 2, 2, 2], [6, 6, 6, 6]), (1, [1, 1, 2, 2], [6, 5, 6, 6]), (2, [1, 1, 1, 2], [6, 5, 5, 6])):
        out = ref.to_cloud(z, K, splat=r, **kw)
        assert out[4].zbuffer.shape == (1, 4) and out[4].zbuffer.reshape(-1).tolist() == want_zb      # nothing beyond the image
        assert out[2].tolist() == want


def test_outside_and_behind_the_colour_camera():
    K = (4.0, 4.0, 1.5, 0.0)
    z = np.ones((1, 4), dtype=np.float32)
    colour = np.full((1, 2, 3), 255, dtype=np.uint8)
    T = np.eye(4)
    T[2, 3] = -1.0                                                   # z' = 0: behind (z' <= 0)
    kw = dict(color=colour, color_intrinsics=(4.0, 4.0, 0.0, 0.0))
    assert ref.to_cloud(z, K, depth_to_color=T, **kw)[2].tolist() == [4, 4, 4, 4]
    # uc = u - 1.5: -1.5, -0.5, 0.5, 1.5 -> fu = -1, 0, 1, 2 against Wc = 2 (floor(-0.5 + 0.5) = 0: inside)
    assert ref.to_cloud(z, K, depth_to_color=np.eye(4), **kw)[2].tolist() == [4, 6, 6, 4]
    T = np.eye(4)
    T[0, 3] = np.nan
    assert ref.to_cloud(z, K, depth_to_color=T, **kw)[2].tolist() == [4, 4, 4, 4]          # a NaN fails the float test


# ---- the synthetic frame ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def frame():
    return ref.synthetic_depth_frame()


def test_synthetic_frame_is_what_it_says(frame):
    assert frame.depth.shape == (480, 640) and frame.depth.dtype == np.uint16
    assert frame.color_aligned.shape == (480, 640, 3) and frame.color.shape == (600, 800, 3) and frame.color.dtype == np.uint8
    assert (np.bincount(frame.ids.reshape(-1) + 1)[1:] > 3000).all()          # the floor, the table and all four boxes are seen
    assert int(frame.is_mixed.sum()) == 1220 and int((frame.depth == 0).sum()) == 15551
    again = ref.synthetic_depth_frame()
    assert np.array_equal(again.depth, frame.depth) and np.array_equal(again.color, frame.color)
    # the table plane of the ray-cast cloud is the table of plane_reference's scene: 0.908 m below the camera
    xyz = ref.to_cloud(**ref.frame_kwargs(frame))[0]
    table = xyz[(frame.ids.reshape(-1) == 1) & np.isfinite(xyz[:, 0])].astype(np.float64)
    height = (np.c_[table, np.ones(len(table))] @ ref.plane_reference.default_transform().T)[:, 2]
    assert abs(np.median(height) - 0.75) < 0.001


def test_registered_mode_with_the_depth_cameras_own_intrinsics_is_aligned_mode(frame):
    aligned = ref.to_cloud(**ref.frame_kwargs(frame, aligned=True))
    same = ref.to_cloud(frame.depth, frame.intrinsics, color=frame.color_aligned, color_intrinsics=frame.intrinsics,
                        depth_to_color=np.eye(4), splat=0, occlusion_margin=0.0)
    assert aligned[3].tolist() == [15551, 0, 0, 0, 0, 0, 291649, 0] == same[3].tolist()
    for a, b in zip(aligned[:2], same[:2]):
        assert np.array_equal(_bits(a), _bits(b))                  # every pixel projects onto itself: fu = u, fv = v
    assert np.array_equal(aligned[2], same[2])


def test_filter_properties_on_the_synthetic_frame(frame):
    """Measured on the reference (seed 5, 640 x 480), edge_threshold t = 0.02 (a jump of 2 % of the nearer depth: 2 cm at 1 m,
    against 1.5 mm noise and at most 9 mm per pixel of slope on the floor):
      * of the 1220 injected mixed pixels 99.18 % are removed;
      * of all other valid0 pixels 2.18 % are removed (the true silhouettes lose one pixel on both sides);
      * with the occlusion test on (margin 0.01, splat 1) 99.91 % of the coloured points take their colour from the surface a
        ray cast from the colour camera sees at that pixel; with it off (margin 1e9) 99.28 %.
    These are properties of the scene and the rule; the bounds leave the margin stated next to each."""
    t = 0.02
    status = ref.to_cloud(**ref.frame_kwargs(frame), edge_threshold=t)[2].reshape(480, 640)
    valid = frame.depth != 0
    mixed, other = frame.is_mixed & valid, valid & ~frame.is_mixed
    removed_mixed, removed_other = float((status[mixed] == 2).mean()), float((status[other] == 2).mean())
    print("mixed removed %.4f, others removed %.4f" % (removed_mixed, removed_other))
    assert removed_mixed >= 0.98                                    # measured 0.9918; margin: 1.2 points
    assert removed_other <= 0.03                                    # measured 0.0218; margin: 0.8 points

    def right_surface(margin):
        out = ref.to_cloud(**ref.frame_kwargs(frame, registered=True), edge_threshold=t, occlusion_margin=margin, details=True)
        vis = out[4].visible.reshape(-1)
        seen = frame.color_ids[out[4].fv.reshape(-1)[vis], out[4].fu.reshape(-1)[vis]]
        return float((frame.ids.reshape(-1)[vis] == seen).mean()), out[3]
    on, counts_on = right_surface(0.01)
    off, counts_off = right_surface(1e9)
    print("right surface: %.4f with the occlusion test, %.4f without" % (on, off), counts_on.tolist())
    assert counts_on.tolist() == [15551, 0, 7549, 0, 650, 2023, 281427, 0] and counts_off[5] == 0
    assert on >= 0.998                                              # measured 0.9991; margin: 0.11 points
    assert off <= 0.995 and on > off                                # measured 0.9928: the test removes 7 in 8 wrong colours


# ---- Python front end and detect's helpers ------------------------------------------------------------------------------------
def test_params_frames_and_npz(tmp_path, frame):
    from regnet_for_3d_grasping_amd import depth_frame as df
    assert df.DepthParams.coerce(None) == df.DepthParams()
    p = df.DepthParams.coerce({"depth_range": [0.2, 3], "edge_threshold": 0.02, "min_neighbours": 2, "splat": 0})
    assert p.depth_range == (0.2, 3.0) and p.edge_threshold == 0.02 and p.occlusion_margin == 0.01 and not p.keep_uncoloured
    assert df.DepthParams.coerce(p) is p
    for bad in ({"min_neighbours": 9}, {"min_neighbours": -1}, {"splat": 3}, {"depth_range": (2, 1)}, {"edge_threshold": -1.0},
                {"occlusion_margin": float("nan")}):
        with pytest.raises(ValueError):
            df.DepthParams.coerce(bad)
    with pytest.raises(TypeError):
        df.DepthParams.coerce(3)
    none = df.DepthFrame(frame.depth, frame.intrinsics)
    aligned = df.DepthFrame(frame.depth, df.Intrinsics(*frame.intrinsics), color=frame.color_aligned)
    registered = df.DepthFrame(**ref.frame_kwargs(frame, registered=True))
    assert (none.mode(), aligned.mode(), registered.mode()) == (0, 1, 2)
    for kw in ({"color": frame.color, "color_intrinsics": frame.color_intrinsics}, {"color": frame.color, "depth_to_color": np.eye(4)},
               {"color_intrinsics": frame.color_intrinsics}):
        with pytest.raises(ValueError):
            df.DepthFrame(frame.depth, frame.intrinsics, **kw).mode()
    # the constants: float64 evaluation, one rounding
    consts = df.pack_params(registered, p, 2)
    assert consts.dtype == np.float32 and consts.shape == (25,)
    assert consts[0] == ref.reciprocal(frame.intrinsics[0]) and consts[4] == f32(0.001) and consts[7] == f32(0.02)
    assert consts[13:22].tolist() == frame.depth_to_color[:3, :3].astype(np.float32).reshape(-1).tolist()
    for fr in (none, aligned, registered):
        path = str(tmp_path / "frame.npz")
        df.save_npz(path, fr)
        back = df.load_npz(path)
        assert back.mode() == fr.mode() and back.intrinsics == fr.intrinsics and back.depth_scale == fr.depth_scale
        assert np.array_equal(back.depth, fr.depth) and back.depth.dtype == np.uint16
        assert (back.color is None) == (fr.color is None) and (fr.color is None or np.array_equal(back.color, fr.color))
        assert back.color_intrinsics == fr.color_intrinsics
    np.savez(str(tmp_path / "bad.npz"), depth=frame.depth)
    with pytest.raises(ValueError):
        df.load_npz(str(tmp_path / "bad.npz"))
    with pytest.raises(RuntimeError, match="GPU"):
        df.to_cloud(none, device="cpu")


def test_detect_helpers():
    from regnet_for_3d_grasping_amd import detect
    ns = argparse.Namespace(depth_range=None, edge_threshold=None, min_neighbours=None, occlusion_margin=None, keep_uncoloured=False)
    assert detect.depth_from_args(ns) is None
    ns = argparse.Namespace(depth_range=[0.2, 2.5], edge_threshold=0.02, min_neighbours=3, occlusion_margin=None, keep_uncoloured=True)
    assert detect.depth_from_args(ns) == {"depth_range": (0.2, 2.5), "edge_threshold": 0.02, "min_neighbours": 3,
                                          "keep_uncoloured": True}
    assert detect.save_path_for("/x/real_data/frame.npz", True) == "/x/real_data_predict/frame.p"
    assert detect.save_path_for("/x/real_data/a.npz.d/frame.npz", True) == "/x/real_data_predict/a.npz.d/frame.p"
    # unchanged: the paths the existing tests use
    assert detect.save_path_for("/x/real_data/frame.pcd", True) == "/x/real_data_predict/frame.p"
    assert detect.save_path_for("/x/test_data/000.p", False) == "/x/test_data_predict/000.p"
    assert detect.save_path_for("/x/plain/000.p", False) == "/x/plain/000.p"
    assert detect.save_path_for("/x/test_data/frame.npz", False) == "/x/test_data_predict/frame.npz"
    assert detect.RESULT_KEYS[0] == "points" and len(detect.RESULT_KEYS) == 7


# ---- the front end's shared pieces: one coerce, one flag table ------------------------------------------------------------------
def _params_classes():
    from regnet_for_3d_grasping_amd import depth_frame, fusion, grasp_select, segment
    return {"select": (grasp_select.SelectParams, False, {"top_k": 5}), "segment": (segment.SegmentParams, False, {"max_objects": 3}),
            "depth": (depth_frame.DepthParams, True, {"depth_range": [0.2, 3], "min_neighbours": 2}),
            "fuse": (fusion.FuseParams, True, {"voxel": 0.005, "origin": [1, 2, 3]})}


@pytest.mark.parametrize("word", ["select", "segment", "depth", "fuse"])
def test_params_coerce(word):
    """None -> None (select, segment) or the defaults (depth, fuse); an instance -> itself; a dict -> the instance of its fields;
    anything else -> a TypeError that names the detector's keyword."""
    cls, none_is_default, fields = _params_classes()[word]
    got = cls.coerce(None)
    assert (got == cls() and type(got) is cls) if none_is_default else got is None
    p = cls()
    assert cls.coerce(p) is p
    q = cls.coerce(fields)
    assert type(q) is cls and q == cls(**fields)
    for key, value in fields.items():
        want = tuple(float(v) for v in value) if isinstance(value, list) else value
        assert getattr(q, key) == want and type(getattr(q, key)) is type(want), key
    for bad in ("x", 3, [1], (1, 2)):
        with pytest.raises(TypeError, match=r"^%s must be None, a dict or a %s$" % (word, cls.__name__)):
            cls.coerce(bad)
    with pytest.raises(TypeError):
        cls.coerce({"no_such_field": 1})


CLI_REQUIRED = ["--folder", "f", "--load-score-path", "s", "--load-region-path", "r"]
CLI_FULL = CLI_REQUIRED + [
    "--top-k", "7", "--nms-translation", "0.02", "--nms-rotation", "15", "--select-from", "grasp_stage2",
    "--auto-table", "--table-range", "0.5", "1.2", "--plane-threshold", "0.004",
    "--depth-range", "0.2", "2.5", "--edge-threshold", "0.02", "--min-neighbours", "3", "--occlusion-margin", "0.02",
    "--keep-uncoloured", "--segment", "--cluster-tolerance", "0.02", "--min-object-points", "30", "--max-objects", "5",
    "--top-k-per-object", "2", "--voxel", "0.004", "--max-voxels", "100", "--min-voxel-points", "2"]
# what the five functions returned for CLI_FULL before they shared one table (printed by a run of that commit)
CLI_FULL_DICTS = {
    "select": {"top_k": 7, "translation_thresh": 0.02, "rotation_thresh_deg": 15.0, "source": "grasp_stage2"},
    "segment": {"tolerance": 0.02, "min_points": 30, "max_objects": 5, "top_k_per_object": 2},
    "transform": {"range": (0.5, 1.2), "threshold": 0.004},
    "depth": {"edge_threshold": 0.02, "min_neighbours": 3, "occlusion_margin": 0.02, "depth_range": (0.2, 2.5),
              "keep_uncoloured": True},
    "fuse": {"voxel": 0.004, "max_voxels": 100, "min_count": 2}}


def test_cli_dicts_of_an_empty_and_a_full_command_line():
    from regnet_for_3d_grasping_amd import detect
    parser = detect.build_parser()
    empty, full = parser.parse_args(CLI_REQUIRED), parser.parse_args(CLI_FULL)
    for name, want in CLI_FULL_DICTS.items():
        from_args = getattr(detect, name + "_from_args")
        assert from_args(empty) is None, name
        got = from_args(full)
        assert got == want and {key: type(value) for key, value in got.items()} == {key: type(value) for key, value in want.items()}, name
    # the switches on their own
    assert detect.transform_from_args(parser.parse_args(CLI_REQUIRED + ["--auto-table"])) == "auto"
    assert detect.segment_from_args(parser.parse_args(CLI_REQUIRED + ["--segment"])) == {}
    assert detect.depth_from_args(parser.parse_args(CLI_REQUIRED + ["--keep-uncoloured"])) == {"keep_uncoloured": True}


def test_help_shows_the_dataclass_defaults():
    """Every numeric default at the end of a flag's help is the default of the field the flag sets."""
    from regnet_for_3d_grasping_amd import detect, table_plane
    classes = {word: entry[0]() for word, entry in _params_classes().items()}
    field_of = {"nms_translation": ("select", "translation_thresh"), "nms_rotation": ("select", "rotation_thresh_deg"),
                "min_neighbours": ("depth", "min_neighbours"), "occlusion_margin": ("depth", "occlusion_margin"),
                "cluster_tolerance": ("segment", "tolerance"), "min_object_points": ("segment", "min_points"),
                "max_objects": ("segment", "max_objects"), "voxel": ("fuse", "voxel"), "max_voxels": ("fuse", "max_voxels"),
                "min_voxel_points": ("fuse", "min_count")}
    seen = set()
    for action in detect.build_parser()._actions:
        shown = re.search(r"\(([-+0-9.einf ]+)\)$", action.help or "")
        if shown is None:
            continue
        seen.add(action.dest)
        values = [float(v) for v in shown.group(1).split()]
        if action.dest == "plane_threshold":
            assert values == [table_plane.DEFAULT_THRESHOLD]
        elif action.dest == "depth_range":
            assert tuple(values) == classes["depth"].depth_range
        else:
            word, field = field_of[action.dest]
            assert values == [getattr(classes[word], field)], action.dest
    assert seen == set(field_of) | {"plane_threshold", "depth_range"}
    by_dest = {action.dest: action.help for action in detect.build_parser()._actions}
    assert by_dest["select_from"].endswith("(%s)" % classes["select"].source)
