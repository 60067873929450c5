"""Pose refinement without a GPU: the header declares csrc/icp.hip's entry points and the binding derives them, the numpy
restatement (tests/icp_reference.py) recovers a known perturbation on the corner scene and reports the scenes that cannot be
registered, ``IcpParams`` refuses what the kernels would, the state block's layout and the CLI's flags."""
import ctypes
import math

import numpy as np
import pytest

from . import icp_reference as ref

_vp, _i64, _int, _f64 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_double
ENTRY_POINTS = {
    "regnet_icp_state_bytes": (_i64, [], []),
    "regnet_icp_workspace_bytes": (_i64, [_i64, _i64], ["N_target", "N_source"]),
    "regnet_icp_prepare_f32": (_int, [_vp, _i64, _f64, _vp, _vp], ["target_xyz", "N_target", "max_dist", "workspace", "stream"]),
    "regnet_icp_step_f32": (_int, [_vp, _i64, _i64, _vp, _i64, _vp, _f64, _vp, _vp, _i64, _vp, _vp],
                            ["source_xyz", "N_source", "stride", "target_normals", "N_target", "state", "max_dist", "idx_out",
                             "sums_out", "min_pairs", "workspace", "stream"]),
}


def test_the_header_declares_the_entry_points_and_the_binding_has_them():
    from regnet_for_3d_grasping_amd import _lib
    for name, (restype, argtypes, names) in ENTRY_POINTS.items():
        assert _lib.SIGNATURES[name] == (restype, argtypes), name
        assert _lib.PARAMS[name] == names, name
        fn = getattr(_lib.lib, name)
        assert fn.restype is restype and list(fn.argtypes) == argtypes, name
        assert _lib.HAS_STREAM[name] == (names[-1:] == ["stream"]), name


def test_host_side_queries_and_refusals_of_the_entry_points():
    """Sizes, and every error that is returned before a launch -- none of these touches a device."""
    from regnet_for_3d_grasping_amd import _lib, registration
    L = _lib.lib
    assert L.regnet_icp_state_bytes() == registration.STATE_BYTES == ref.STATE_BYTES == 128 + 16 * 64
    grid = lambda n: (16 * 4 + 65537 * 4 + 15) // 16 * 16 + 16 * n          # csrc/grid.h: header, cell starts, float4 rows
    for nt, ns in ((0, 0), (1, 1), (1000, 257), (5, 256), (1 << 21, 1 << 21)):
        assert L.regnet_icp_workspace_bytes(nt, ns) == grid(nt) + max(1, -(-ns // 256)) * 256, (nt, ns)
    for nt, ns in ((-1, 0), (0, -1), ((1 << 21) + 1, 0), (0, (1 << 21) + 1)):
        assert L.regnet_icp_workspace_bytes(nt, ns) == -1
    one = ctypes.c_void_p(16)                                                # a non-NULL pointer that is never followed
    assert L.regnet_icp_prepare_f32(one, -1, 0.02, one, None) == -1
    assert L.regnet_icp_prepare_f32(one, (1 << 21) + 1, 0.02, one, None) == -3
    for bad in (0.0, -1.0, float("inf"), float("nan"), 1e-60, 1e60):
        assert L.regnet_icp_prepare_f32(one, 4, bad, one, None) == -3, bad
    assert L.regnet_icp_prepare_f32(None, 4, 0.02, one, None) == -2 and L.regnet_icp_prepare_f32(one, 4, 0.02, None, None) == -2
    step = lambda **kw: L.regnet_icp_step_f32(*[kw.get(k, v) for k, v in (
        ("src", one), ("ns", 4), ("stride", 1), ("nrm", one), ("nt", 4), ("state", one), ("dist", 0.02), ("idx", None),
        ("sums", None), ("min_pairs", 1), ("ws", one), ("stream", None))])
    assert step(ns=-1) == step(nt=-1) == step(stride=0) == step(min_pairs=-1) == -1
    assert step(ns=(1 << 21) + 1) == step(nt=(1 << 21) + 1) == step(dist=0.0) == step(dist=float("nan")) == -3
    assert step(src=None) == step(nrm=None) == step(state=None) == step(ws=None) == -2


def test_the_build_compiles_icp_with_individual_roundings_and_checks_its_registers():
    import importlib.util
    import os
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "regnet_for_3d_grasping_amd", "csrc", "build.py")
    spec = importlib.util.spec_from_file_location("regnet_build_for_icp_test", path)
    build = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(build)
    assert dict(build.SOURCES)["icp.hip"] == ["-ffp-contract=off"]
    assert build.NO_VGPR_SPILL["icp.o"] == ["icp_"]


@pytest.fixture(scope="module")
def corner():
    target, normals = ref.corner_scene()
    truth = ref.perturbation(2.5, 7.0)
    return target, normals, truth, ref.moved_source(target, truth)


def test_the_restatement_recovers_a_known_perturbation_on_the_corner_scene(corner):
    target, normals, truth, source = corner
    assert target.shape == (1723, 3) and source.shape == (575, 3) and target.dtype == source.dtype == np.float32
    out = ref.icp(source, target, normals, None, {"max_dist": 0.02})
    print("status %d after %d iterations, pairs %d, rms %.3g -> %.3g, pose error %.3g" % (
        out["status"], out["iterations"], out["pairs"], out["rms_first"], out["rms_last"], ref.pose_distance(out["pose"], truth)))
    assert out["status"] == ref.CONVERGED and out["iterations"] <= 6
    assert (out["history"][:, 0] == 575).all()                               # every row matched in every iteration
    assert 1e-3 < out["rms_first"] < 7e-3                                    # the perturbation moves a point by at most ~ 1 cm
    # the source is the moved target rounded to float32: half an ulp of 0.2 m, 7.5e-9, is the noise; a point-to-plane residual
    # cannot go below it nor should it stay more than a few times above
    assert out["rms_last"] < 4 * 7.5e-9
    assert ref.pose_distance(out["pose"], truth) < 8 * 7.5e-9
    # from the truth itself nothing moves: one step, converged
    again = ref.icp(source, target, normals, truth, {"max_dist": 0.02})
    assert again["status"] == ref.CONVERGED and again["iterations"] == 1 and ref.pose_distance(again["pose"], truth) < 8 * 7.5e-9


def test_ties_thresholds_and_skipped_rows_of_the_correspondence():
    target = np.array([[0, 0, 0], [0.25, 0, 0], [0.25, 0, 0], [np.nan, 0, 0], [1, 1, 1]], dtype=np.float32)
    source = np.array([[0.125, 0, 0], [0.25, 0, 0], [np.inf, 0, 0], [0.5, 0, 0], [3, 3, 3]], dtype=np.float32)
    idx, _ = ref.correspond(source, target, np.eye(4), 0.25)
    assert idx.tolist() == [0, 1, -2, 1, -1]                 # equidistant -> row 0; duplicates -> the lower; exactly max_dist
    idx, _ = ref.correspond(source, target, np.eye(4), float(np.nextafter(np.float32(0.25), np.float32(0)))  )
    assert idx.tolist() == [0, 1, -2, -1, -1]
    idx, _ = ref.correspond(source, target, np.eye(4), 0.25, stride=2)
    assert idx.tolist() == [0, -2, -1]
    assert ref.max_dist2(0.02) == np.float32(0.02 * 0.02) and ref.max_dist2(0.02).dtype == np.float32


@pytest.mark.parametrize("planes", [1, 2])
def test_planes_that_leave_a_motion_free_are_degenerate_and_the_pose_is_untouched(planes):
    """One plane leaves three motions free, two planes sharing an edge the slide along it: the caller must be told."""
    target, normals = ref.corner_scene(planes, 0)
    init = ref.perturbation(1.0, 3.0)
    source = ref.moved_source(target, ref.perturbation(2.5, 7.0))
    out = ref.icp(source, target, normals, init, {"max_dist": 0.02, "min_pairs": 10})
    assert out["status"] == ref.DEGENERATE and out["iterations"] == 1 and out["pairs"] >= 10
    assert out["pose"].tobytes() == np.array(init, dtype=np.float64).tobytes()
    few = ref.icp(source, target, normals, init, {"max_dist": 0.02, "min_pairs": 10000})
    assert few["status"] == ref.TOO_FEW and few["pose"].tobytes() == np.array(init, dtype=np.float64).tobytes()


def test_the_solve_against_numpy_and_the_small_angle_branch():
    rng = np.random.RandomState(0)
    A = rng.normal(size=(40, 6))
    H, g = A.T @ A, rng.normal(size=6)
    x = ref.cholesky_solve(H, g)
    assert np.allclose(x, np.linalg.solve(H, -g), rtol=1e-10, atol=0)
    H[4, :] = H[:, 4] = 0.0
    assert ref.cholesky_solve(H, g) is None
    for w in ([1e-9, 2e-9, -1e-9], [0.3, -0.2, 0.1], [0.0, 0.0, 0.0]):
        R = ref.rodrigues(w)
        assert np.abs(R @ R.T - np.eye(3)).max() < 1e-15 and abs(np.linalg.det(R) - 1.0) < 1e-15
    th = 0.37
    assert np.allclose(ref.rodrigues([0, 0, th]), [[math.cos(th), -math.sin(th), 0], [math.sin(th), math.cos(th), 0], [0, 0, 1]],
                       rtol=0, atol=1e-16)


def test_icp_params_refusals_and_the_state_block():
    from regnet_for_3d_grasping_amd import registration
    P = registration.IcpParams
    d = P()
    assert (d.max_dist, d.iterations, d.stride, d.min_pairs) == (0.02, 30, 1, 100)
    assert {k: getattr(d, k) for k in ref.DEFAULTS} == ref.DEFAULTS
    assert P.coerce(None) is None and P.coerce({"stride": 4}).stride == 4 and P.coerce(d) is d
    with pytest.raises(TypeError, match="register"):
        P.coerce("yes")
    for bad in ({"max_dist": 0.0}, {"max_dist": float("nan")}, {"max_dist": 1e60}, {"iterations": 0}, {"iterations": 65},
                {"iterations": 2.5}, {"stride": 0}, {"min_pairs": -1}, {"rot_eps": -1.0}, {"trans_eps": float("inf")},
                {"normal_radius": 0.0}, {"normal_max_nn": 2}, {"normal_max_nn": 65}):
        with pytest.raises(ValueError, match="register"):
            P(**bad)
    with pytest.raises(TypeError):
        P(voxel=1.0)
    init = ref.perturbation(1.0, 2.0)
    raw = registration.initial_state(init, {"iterations": 7, "rot_eps": 1e-4, "trans_eps": 2e-4})
    assert raw.dtype == np.uint8 and raw.shape == (registration.STATE_BYTES,)
    assert raw[:96].view(np.float64).tobytes() == init[:3].tobytes()
    assert raw[96:112].view(np.int32).tolist() == [0, 0, 7, 0] and raw[112:128].view(np.float64).tolist() == [1e-4, 2e-4]
    assert not raw[128:].any()
    got = registration.decode_state(raw)
    assert got["pose"].tobytes() == init.tobytes() and (got["status"], got["iterations"], got["pairs"]) == (0, 0, 0)
    raw[96:104].view(np.int32)[:] = (2, registration.CONVERGED)
    raw[128:160].view(np.float64)[:] = (575.0, 3e-3, 570.0, 1e-5)
    got = registration.decode_state(raw)
    assert registration.report_row(got) == [1.0, 2.0, 570.0, 3e-3, 1e-5]
    with pytest.raises(ValueError):
        registration.initial_state(np.eye(3))
    assert registration.STATUS_NAMES[registration.DEGENERATE] == "DEGENERATE"
    assert (ref.RUNNING, ref.CONVERGED, ref.MAX_ITER, ref.TOO_FEW, ref.DEGENERATE) == (
        registration.RUNNING, registration.CONVERGED, registration.MAX_ITER, registration.TOO_FEW, registration.DEGENERATE)


def test_the_cli_turns_registration_on_and_the_detector_keys():
    from regnet_for_3d_grasping_amd import detect
    required = ["--folder", "x", "--load-score-path", "a", "--load-region-path", "b"]
    parser = detect.build_parser()
    assert detect.register_from_args(parser.parse_args(required)) is None
    assert detect.register_from_args(parser.parse_args(required + ["--refine-poses"])) == {}
    got = detect.register_from_args(parser.parse_args(required + ["--icp-distance", "0.01", "--icp-iterations", "12",
                                                                  "--icp-stride", "4"]))
    assert got == {"max_dist": 0.01, "iterations": 12, "stride": 4}
    assert detect.REGISTER_KEYS == ("fuse_poses", "fuse_register")
    parser.format_help()
