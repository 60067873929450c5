"""Table-plane estimation without a GPU: the C ABI's new entry points (exported, declared, argument checks before any launch),
the numpy restatement of the contract (tests/plane_reference.py) against answers derived by hand, ``table_frame``'s properties,
and the recovery of the default camera pose from a seeded synthetic frame."""
import argparse
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

from . import plane_reference as ref

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("regnet_plane_workspace_bytes", "regnet_plane_estimate_f32", "regnet_plane_estimate_f64")
MAX_M, MAX_H = 1 << 21, 4096


def test_new_symbols_are_exported_bound_and_declared():
    from regnet_for_3d_grasping_amd import _lib
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "regnet_hip.h")).read(), flags=re.S)
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert hasattr(raw, name), name
        assert name in _lib.SIGNATURES, name
        assert re.search(r"\b%s\s*\(" % name, header), name
    assert len(_lib.SIGNATURES["regnet_plane_estimate_f32"][1]) == 17 == len(_lib.SIGNATURES["regnet_plane_estimate_f64"][1])
    assert _lib.lib.regnet_abi_version() == 2


@pytest.mark.parametrize("name", NEW_SYMBOLS[1:])
def test_argument_checks_without_gpu(name):
    from regnet_for_3d_grasping_amd import _lib
    fn = getattr(_lib.lib, name)

    def call(M, H, ptr=1, ws=1, stages=15):
        # validation happens before any launch, so these are safe without a device
        return fn(ptr, M, H, 0, 0.005, 0.0, math.inf, None, 0.0, ptr, ptr, ptr, ptr, ptr, ws, stages, None)
    assert call(-1, 1024) == -1                                   # negative M
    for H in (0, -64, 1, 63, 100, 1000):
        assert call(100, H) == -1, H                              # H not a positive multiple of 64
    assert call(100, 1024, stages=0) == -1 and call(100, 1024, stages=16) == -1
    assert call(MAX_M + 1, 1024) == -3                            # M > 2^21
    assert call(100, MAX_H + 64) == -3                            # H > 4096
    assert call(100, 1024, ptr=None) == -2                        # null pointers ...
    assert call(100, 1024, ws=None) == -2                         # ... the workspace among them
    assert call(MAX_M, MAX_H, ptr=None) == -2                     # the limits themselves are supported


def test_workspace_size_formula():
    from regnet_for_3d_grasping_amd import _lib, table_plane
    ws = _lib.lib.regnet_plane_workspace_bytes
    for M in (0, 1, 100003, MAX_M):
        for H in (64, 128, 1024, MAX_H):
            assert ws(M, H) == 32 * H == table_plane.workspace_bytes(M, H)
    for M, H in ((-1, 64), (MAX_M + 1, 64), (10, 0), (10, 65), (10, MAX_H + 64), (10, -64)):
        assert ws(M, H) == -1
    assert table_plane.MAX_FRAME_POINTS == MAX_M and table_plane.MAX_HYPOTHESES == MAX_H


def test_generator_known_answers():
    # splitmix64's published first outputs for the state 0 (the reference implementation's test vector) and for 1234567
    assert ref.splitmix64(0) == 0xE220A8397B1DCDAF
    assert ref.splitmix64(0x9E3779B97F4A7C15) == 0x6E789E6AA1B965F4
    assert ref.splitmix64(1234567) == 6457827717110365317
    # the row is the high word scaled by M: always in [0, M)
    for M in (1, 2, 63, 100003, MAX_M):
        rows = [ref.draw_row(3, h, k, r, M) for h in (0, 1, 4095) for k in range(3) for r in range(8)]
        assert min(rows) >= 0 and max(rows) < M
    assert ref.draw_row(0, 0, 0, 0, 1 << 32) == ref.splitmix64(0) >> 32
    assert ref.draw_row(1, 2, 1, 3, 1 << 32) == ref.splitmix64((1 << 32) + (3 * 2 + 1) * 8 + 3) >> 32


def _grid(z, nx=8, ny=8, x0=0.0):
    gx, gy = np.meshgrid(np.arange(nx) / 8.0 + x0, np.arange(ny) / 8.0)
    return np.stack([gx.ravel(), gy.ravel(), np.full(nx * ny, z)], axis=1).astype(np.float32)


def test_coplanar_grid_every_point_is_an_inlier_of_every_valid_hypothesis():
    xyz = _grid(1.0)                       # coordinates on the 1/8 grid: every product and sum below is exact
    out = ref.estimate_plane(xyz, H=64)
    table, counts = out["table"], out["counts"]
    valid = table[:, 7] == 2.0
    assert 32 < valid.sum() < 64           # collinear and repeated draws are invalid
    assert (table[valid, 0] == 0).all() and (table[valid, 1] == 0).all() and (table[valid, 2] != 0).all()
    assert (counts[valid] == 64).all() and (counts[~valid] == -1).all()
    assert out["winner"] == int(np.nonzero(valid)[0][0]) and out["count"] == 64        # the tie goes to the lowest index
    assert out["mask"].all()
    assert np.allclose(np.abs(out["normal"]), [0, 0, 1]) and out["normal"][2] < 0 and abs(out["offset"] + 1.0) < 1e-12
    assert out["rms"] < 1e-7


def test_point_exactly_at_the_threshold_is_included():
    t = 2.0 ** -8
    row = np.array([0, 0, 2, 0, 0, 0, 4, 2], dtype=np.float32)                  # n = (0,0,2), p0 = 0, nn = 4
    above = np.float32(t) * (np.float32(1) + np.float32(2.0 ** -23))
    p = np.array([[0.3, 0.2, t], [0.3, 0.2, -t], [0.3, 0.2, above], [0.1, 0.7, 0.0], [np.nan, 0, 0]], dtype=np.float32)
    mask = ref.inlier_mask(p, np.isfinite(p).all(axis=1), row, t)
    assert mask.tolist() == [True, True, False, True, False]                    # s s = 2^-14 = (t t) nn: inclusive


def test_collinear_points_give_no_plane():
    xyz = np.stack([np.arange(50) / 8.0, np.zeros(50), np.ones(50)], axis=1).astype(np.float32)
    out = ref.estimate_plane(xyz, H=64)
    assert (out["table"][:, 7] == 0).all() and (out["table"][:, 6] == 0).all()
    assert (out["counts"] == -1).all() and out["winner"] == -1 and out["count"] == 0 and not out["mask"].any()


def test_all_nan_gives_no_plane():
    out = ref.estimate_plane(np.full((100, 3), np.nan, dtype=np.float32), H=64)
    assert not out["table"].any()                                               # unfilled slots: zero rows
    assert (out["counts"] == -1).all() and out["winner"] == -1 and not out["mask"].any()
    out = ref.estimate_plane(np.zeros((0, 3), dtype=np.float32), H=64)
    assert out["winner"] == -1 and not out["table"].any() and out["mask"].shape == (0,)


def test_retry_rule_takes_the_first_finite_attempt():
    M = 1000
    finite = np.zeros(M, dtype=bool)
    attempts = [ref.draw_row(7, 5, 1, r, M) for r in range(8)]
    finite[attempts[3]] = True
    want = next(r for r in range(8) if attempts[r] == attempts[3])
    idx = ref.draw_triples(7, 64, M, finite)
    assert idx[5, 1] == attempts[want]
    finite[:] = False
    assert (ref.draw_triples(7, 64, M, finite) == -1).all()


def test_tie_goes_to_the_lower_index():
    assert ref.select(np.array([5, 9, 9, 3], dtype=np.int32)) == (1, 9)
    assert ref.select(np.array([-1, 2, 2, -1], dtype=np.int32)) == (-1, 0)      # fewer than 3 inliers: no plane
    assert ref.select(np.array([-1, -1, 3, 3], dtype=np.int32)) == (2, 3)


def test_range_gate_excludes_the_larger_plane():
    xyz = np.concatenate([_grid(1.0, 16, 16), _grid(2.0, 24, 16, x0=-1.0)])     # 256 points at distance 1, 384 at distance 2
    plain = ref.estimate_plane(xyz, H=128)
    assert plain["count"] == 384 and abs(plain["offset"] + 2.0) < 1e-9
    gated = ref.estimate_plane(xyz, H=128, range=(0.5, 1.5))
    assert gated["count"] == 256 and abs(gated["offset"] + 1.0) < 1e-9
    assert (gated["table"][:, :7] == plain["table"][:, :7]).all()               # the gate changes flags and counts only
    assert (gated["table"][:, 7] <= plain["table"][:, 7]).all() and (gated["table"][:, 7] == 1.0).any()
    assert (gated["counts"][gated["table"][:, 7] != 2.0] == -1).all()
    # the tilt gate: planes within 10 degrees of the camera's z axis only -- both horizontal planes pass, mixed triples do not
    tilt = ref.estimate_plane(xyz, H=128, up_hint=(0, 0, 1), max_tilt_deg=10.0)
    assert tilt["count"] == 384 and (tilt["table"][:, 7] == 1.0).any()
    steep = ref.estimate_plane(xyz, H=128, up_hint=(1, 0, 0), max_tilt_deg=10.0)
    assert steep["winner"] == -1 or steep["count"] <= 40          # a plane that cuts both grids meets each in one line


def _frames():
    from regnet_for_3d_grasping_amd import table_plane
    return (table_plane.table_frame, lambda plane, height=0.75: ref.table_frame(plane[0], plane[1], height))


@pytest.mark.parametrize("which", [0, 1], ids=["package", "reference"])
def test_table_frame_properties(which):
    frame = _frames()[which]
    rng = np.random.RandomState(11)
    for _ in range(50):
        n = rng.normal(size=3)
        n /= np.linalg.norm(n)
        offset = -rng.uniform(0.3, 2.0)
        height = rng.uniform(0.0, 1.0)
        T = frame((n, offset), height)
        R = T[:3, :3]
        assert T.dtype == np.float64 and T.shape == (4, 4) and (T[3] == [0, 0, 0, 1]).all()
        assert np.abs(R @ R.T - np.eye(3)).max() < 1e-12 and abs(np.linalg.det(R) - 1.0) < 1e-12
        assert np.abs(R[2] - n).max() < 1e-12
        # points of the plane n . x = offset land at z = table_height
        basis = np.linalg.svd(n[None, :])[2][1:]
        pts = offset * n + rng.normal(size=(20, 2)) @ basis
        assert np.abs((pts @ R.T + T[:3, 3])[:, 2] - height).max() < 1e-12
        # the camera origin lands above the frame's origin, at its distance to the plane above the table
        assert T[0, 3] == 0 and T[1, 3] == 0 and abs(T[2, 3] - (height - offset)) < 1e-12
        assert abs(R[0] @ np.array([1.0, 0, 0])) > 0 and abs(R[0] @ n) < 1e-12    # x' is the projected camera x axis


@pytest.mark.parametrize("which", [0, 1], ids=["package", "reference"])
def test_table_frame_across_the_axis_fallback(which):
    """The camera's x axis projected into the plane is shorter than 1e-6 when the normal is within 1e-6 rad of +-x: the y axis
    takes over.  On both sides of the switch the frame is a rotation with z' = the normal and the same translation, so the
    plane's height and the camera's position -- what the crop's z test and the collision filter read -- pass through it
    continuously; x' itself cannot (it turns from x to y)."""
    frame = _frames()[which]
    last = None
    for angle in (3e-6, 1.5e-6, 0.9e-6, 0.5e-6, 0.0):
        n = np.array([math.cos(angle), 0.0, -math.sin(angle)])
        T = frame((n, -1.25), 0.75)
        R = T[:3, :3]
        assert np.abs(R @ R.T - np.eye(3)).max() < 1e-9 and abs(np.linalg.det(R) - 1.0) < 1e-9
        assert np.abs(R[2] - n).max() < 1e-12 and abs(T[2, 3] - 2.0) < 1e-12
        if angle >= 1e-6:
            assert abs(R[0, 2]) > 0.99            # the projection of x: along -+z of the camera
        else:
            assert abs(R[0, 1]) > 0.99            # the fallback: the camera's y axis
        if last is not None:
            assert np.abs(T[2] - last[2]).max() < 2e-6
        last = T


def test_default_transform_restated():
    from regnet_for_3d_grasping_amd import ingest, table_plane
    T = ingest.table_frame_transform()
    assert np.abs(ref.default_transform() - T).max() < 1e-15
    # the default transform IS the table frame of the plane it puts at z = 0.75
    assert np.abs(table_plane.table_frame((T[2, :3], 0.75 - T[2, 3]), 0.75) - T).max() < 1e-15


@pytest.fixture(scope="module")
def recovered():
    xyz, _ = ref.synthetic_frame()
    return xyz, ref.estimate_plane(xyz, range=(0.5, 1.2)), ref.estimate_plane(xyz)


def test_recovery_on_the_synthetic_frame(recovered):
    from regnet_for_3d_grasping_amd import table_plane
    xyz, gated, plain = recovered
    finite = int(np.isfinite(xyz).all(axis=1).sum())
    assert len(xyz) == 640 * 480 and finite == 214949
    assert (plain["table"][:, 7] == 2.0).all()                   # the 8-attempt retry rule fills every slot at 30 % holes
    # ungated, the floor wins by a wide margin: the gate is part of the contract
    assert plain["count"] == 125454 and abs(-plain["offset"] - 1.658) < 0.01
    assert abs(-gated["offset"] - (1.658 - 0.75)) < 0.002 and gated["count"] > 50000
    T = table_plane.table_frame((gated["normal"], gated["offset"]))
    assert np.abs(T - ref.table_frame(gated["normal"], gated["offset"])).max() < 1e-15
    error = np.abs(T - ref.default_transform())
    print("recovered transform: max |rotation error| %.3g, |translation error| %.3g, rms %.4g mm, %d inliers" % (
        error[:3, :3].max(), error[:3, 3].max(), gated["rms"] * 1e3, gated["count"]))
    # measured on this seed: rotation entries within 3.0004e-05, camera height within 4.359e-07 m, rms 1.489 mm.  The bounds are
    # twice that: a property of the 1.5 mm noise over 84 345 inliers, not of the code under test
    assert error[:3, :3].max() < 2 * 3.0004e-05
    assert error[:3, 3].max() < 2 * 4.359e-07
    assert abs(gated["rms"] - 0.0015) < 0.0001


def test_python_argument_checks():
    from regnet_for_3d_grasping_amd import table_plane
    with pytest.raises(RuntimeError, match="CUDA tensor"):
        table_plane.estimate_device(torch.zeros(10, 3))
    assert table_plane.cos2_tilt(60.0) == float(np.float32(math.cos(math.radians(60.0)) ** 2))
    m = ref.moments_of(*(lambda p: (p, np.ones(len(p), dtype=bool)))(_grid(1.0)))[0]
    plane = table_plane.plane_from_moments(m, 3, 64)
    assert plane.hypothesis == 3 and plane.inliers == 64 and abs(plane.offset + 1.0) < 1e-12 and plane.normal[2] < 0


def test_cli_flags_turn_the_estimation_on():
    from regnet_for_3d_grasping_amd import detect
    ns = argparse.Namespace(auto_table=False, table_range=None, plane_threshold=None)
    assert detect.transform_from_args(ns) is None
    ns.auto_table = True
    assert detect.transform_from_args(ns) == "auto"
    ns = argparse.Namespace(auto_table=False, table_range=[0.5, 1.2], plane_threshold=0.004)
    assert detect.transform_from_args(ns) == {"range": (0.5, 1.2), "threshold": 0.004}
    assert detect.TABLE_KEYS == ("table_transform", "table_plane")
