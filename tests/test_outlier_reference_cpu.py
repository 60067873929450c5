"""The outlier filters without a GPU: the header's four prototypes and their binding, the build entry, ``OutlierParams``, the CLI's
flags, and the numpy restatement (tests/outlier_reference.py) against hand-built cases, against scipy's k-d tree where scipy is
importable, and on a rendered scene with planted speckle."""
import math

import numpy as np
import pytest

from . import outlier_reference as ref

f32 = np.float32
NEW = ("regnet_outlier_workspace_bytes", "regnet_outlier_radius_f32", "regnet_outlier_knn_f32", "regnet_outlier_stats_f64")
REQUIRED = ["--folder", "x", "--load-score-path", "a", "--load-region-path", "b"]


def test_the_header_declares_the_prototypes_and_the_build_lists_the_source():
    import ctypes
    from regnet_for_3d_grasping_amd import _lib
    from regnet_for_3d_grasping_amd.csrc import build
    with open(_lib.HEADER_PATH) as f:
        signatures, _ = _lib.parse_header(f.read())
    for name in NEW:
        assert name in signatures and signatures[name] == _lib.SIGNATURES[name] and hasattr(_lib.lib, name)
    assert _lib.PARAMS["regnet_outlier_radius_f32"] == ["xyz", "mask", "N", "radius", "min_neighbours", "count", "workspace", "stream"]
    assert _lib.PARAMS["regnet_outlier_knn_f32"] == ["xyz", "mask", "N", "k", "max_radius", "mean_dist", "found", "workspace", "stream"]
    assert _lib.SIGNATURES["regnet_outlier_workspace_bytes"] == (ctypes.c_int64, [ctypes.c_int64])
    assert _lib.SIGNATURES["regnet_outlier_radius_f32"][1][3] is ctypes.c_float
    assert dict(build.SOURCES)["outlier.hip"] == ["-ffp-contract=off"]
    assert build.NO_VGPR_SPILL["outlier.o"] == ["outlier_"]
    from regnet_for_3d_grasping_amd import outliers
    assert outliers.workspace_bytes(-1) == outliers.workspace_bytes(1 << 31) == -1
    assert outliers.workspace_bytes(0) > 0 and outliers.workspace_bytes(1000) - outliers.workspace_bytes(0) == 1000 * (4 + 12 + 16)


def test_outlier_params_defaults_and_refusals():
    from regnet_for_3d_grasping_amd import outliers
    P = outliers.OutlierParams
    d = P()
    assert (d.mode, d.radius, d.min_neighbours, d.knn, d.max_radius, d.std_ratio) == ("radius", 0.04, 16, 20, 0.04, 2.0)
    assert P.coerce(None) is None and P.coerce(d) is d and P.coerce({"mode": "both", "knn": 64}) == P(mode="both", knn=64)
    for bad in ({"mode": "median"}, {"radius": 0.0}, {"radius": -1.0}, {"radius": math.inf}, {"radius": math.nan}, {"radius": 1e-60},
                {"max_radius": 0.0}, {"max_radius": 1e60}, {"min_neighbours": 0}, {"knn": 0}, {"knn": 65}, {"std_ratio": -0.5},
                {"std_ratio": math.nan}, {"std_ratio": math.inf}):
        with pytest.raises(ValueError, match="denoise"):
            P(**bad)
    with pytest.raises(TypeError, match=r"^denoise must be None, a dict or a OutlierParams$"):
        P.coerce(3)
    assert "Nobody has measured" in " ".join(P.__doc__.split())


def test_the_cli_flags_reach_outliers_from_args():
    from regnet_for_3d_grasping_amd import detect, outliers
    parser = detect.build_parser()
    assert detect.outliers_from_args(parser.parse_args(REQUIRED)) is None
    assert detect.outliers_from_args(parser.parse_args(REQUIRED + ["--denoise"])) == {}
    got = detect.outliers_from_args(parser.parse_args(REQUIRED + [
        "--outlier-mode", "both", "--outlier-radius", "0.03", "--outlier-min-neighbours", "8", "--outlier-knn", "12",
        "--outlier-max-radius", "0.05", "--outlier-std-ratio", "1.5"]))
    want = {"mode": "both", "radius": 0.03, "min_neighbours": 8, "knn": 12, "max_radius": 0.05, "std_ratio": 1.5}
    assert got == want and {k: type(v) for k, v in got.items()} == {k: type(v) for k, v in want.items()}
    assert outliers.OutlierParams.coerce(got) == outliers.OutlierParams(**want)
    with pytest.raises(SystemExit):
        parser.parse_args(REQUIRED + ["--outlier-mode", "median"])
    assert detect.DENOISE_KEYS == ("denoise_num",)
    helps = {a.dest: a.help for a in parser._actions}
    assert helps["outlier_mode"].endswith("(radius)") and "(0.04 m)" in helps["outlier_radius"] and "(16 points)" in helps["outlier_min_neighbours"]
    parser.format_help()


# ---- the restatement against answers derived by hand ------------------------------------------------------------------------------
def _lattice(n, step=0.25):
    g = np.arange(n, dtype=np.float32) * f32(step)         # multiples of 2^-2: every difference and d2 is exact
    return np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3)


def test_a_lattice_has_the_known_counts():
    """5 x 5 x 5 points 0.25 apart, radius 0.25 (inclusive): the face neighbours, 6 inside, 5 on a face, 4 on an edge, 3 at a
    corner; radius 0.36 > 0.25 sqrt 2 adds the 12 edge neighbours inside."""
    pts = _lattice(5)
    on_border = ((pts == 0) | (pts == 1.0)).sum(axis=1)
    count = ref.radius_count(pts, None, 0.25, 100)
    assert np.array_equal(count, 6 - on_border)
    assert ref.radius_count(pts, None, 0.36, 100)[on_border == 0].tolist() == [18] * 27
    assert np.array_equal(ref.radius_count(pts, None, 0.25, 4), np.minimum(6 - on_border, 4))        # saturated
    mean, found = ref.knn_mean_distance(pts, None, 6, 0.25)
    assert np.array_equal(found, 6 - on_border)
    assert np.array_equal(mean[on_border == 0], np.full(27, 0.25, dtype=np.float32)) and np.isnan(mean[on_border > 0]).all()
    assert mean[on_border > 0].view(np.uint32).tolist() == [ref.QNAN_BITS] * int((on_border > 0).sum())


def test_exactly_min_neighbours_and_one_fewer():
    centre = np.zeros((1, 3), dtype=np.float32)
    ring = np.array([[0.03 * math.cos(a), 0.03 * math.sin(a), 0.0] for a in np.linspace(0, 2 * math.pi, 16, endpoint=False)], dtype=np.float32)
    far = ring * f32(40.0)                                  # 1.2 m out, > 0.2 m apart: no neighbour of anything
    full = np.concatenate([centre, ring, far])
    out = ref.filter_cloud(full, "radius")
    assert out["count"][0] == 16 and out["keep"][0] and out["status"][0] == ref.KEPT
    assert (out["count"][17:] == 0).all() and (out["status"][17:] == ref.TOO_FEW_IN_RADIUS).all()
    out = ref.filter_cloud(full[np.arange(len(full)) != 5], "radius")
    assert out["count"][0] == 15 and not out["keep"][0] and out["status"][0] == ref.TOO_FEW_IN_RADIUS
    assert out["num"].tolist() == np.bincount(out["status"], minlength=5).tolist() and out["num"].sum() == len(full) - 1


def test_duplicates_count_and_the_row_itself_does_not():
    pts = np.zeros((5, 3), dtype=np.float32)
    pts[4] = [1.0, 0.0, 0.0]
    assert ref.radius_count(pts, None, 0.01, 10).tolist() == [3, 3, 3, 3, 0]
    mean, found = ref.knn_mean_distance(pts, None, 3, 0.01)
    assert found.tolist() == [3, 3, 3, 3, 0] and mean[:4].tolist() == [0.0] * 4 and np.isnan(mean[4])
    masked = ref.radius_count(pts, np.array([1, 0, 1, 1, 1]), 0.01, 10)
    assert masked.tolist() == [2, -1, 2, 2, 0]
    pts[2, 1] = np.nan
    assert ref.radius_count(pts, None, 0.01, 10).tolist() == [2, 2, -1, 2, 0]


def test_the_threshold_is_inclusive_at_one_ulp():
    R = f32(0.25)
    R2 = R * R
    outside = np.nextafter(R2, f32(np.inf))
    # d2 = dx^2 + dy^2 with dx = 0.25 (d2 == R2 alone), and dy^2 = one ulp of R2 added (2^-28 = (2^-14)^2)
    assert outside - R2 == f32(2.0 ** -27)
    pts = np.array([[0, 0, 0], [0.25, 0, 0]], dtype=np.float32)
    assert ref.radius_count(pts, None, R, 5).tolist() == [1, 1]
    assert f32(ref.d2_block(pts[:1], pts[1:])[0, 0]) == R2
    # one ulp beyond: dx = 0.25 + 2^-13 -> dx^2 = R2 + 2^-14 + 2^-26, far outside; the pair at one ulp on the device's lattice
    # is built in tests/test_gpu_outliers.py and checked here through its own assertions
    from . import test_gpu_outliers as device_cases
    cloud, R = device_cases._threshold_cloud()
    assert ref.radius_count(cloud, None, R, 3).tolist() == [2, 1, 1, 0]


def test_statistics_of_fewer_than_two_rows_and_the_two_pass_deviation():
    n, mu, sigma, thr = ref.stats(np.array([], dtype=np.float32), np.array([], dtype=np.int32), 3, 2.0)
    assert n == 0 and math.isnan(mu) and math.isnan(sigma) and thr == np.inf
    n, mu, sigma, thr = ref.stats(np.array([0.5, 9.0], dtype=np.float32), np.array([3, 2], dtype=np.int32), 3, 2.0)
    assert n == 1 and mu == 0.5 and math.isnan(sigma) and thr == np.inf
    n, mu, sigma, thr = ref.stats(np.array([0.25, 0.75], dtype=np.float32), np.array([3, 3], dtype=np.int32), 3, 2.0)
    assert (n, mu) == (2, 0.5) and sigma == math.sqrt(0.125) and thr == f32(0.5 + 2.0 * math.sqrt(0.125))
    assert ref.stats(np.array([0.25, 0.75], dtype=np.float32), np.array([3, 3], dtype=np.int32), 3, 0.0)[3] == f32(0.5)
    rng = np.random.RandomState(3)
    m = (1.0 + 1e-6 * rng.standard_normal(1000)).astype(np.float32)
    _, _, sigma, _ = ref.stats(m, np.full(1000, 3), 3, 2.0)
    exact = math.sqrt(sum((float(v) - math.fsum(m.astype(np.float64)) / 1000) ** 2 for v in m) / 999)
    assert abs(sigma - exact) <= 1e-9 * exact
    one_pass = math.sqrt(abs(float((m.astype(np.float64) ** 2).sum()) - 1000 * float(m.astype(np.float64).mean()) ** 2) / 999)
    assert abs(one_pass - exact) > 1e-6 * exact              # the form the contract rules out loses the spread


def test_status_rules_and_both():
    """A dense blob, a sparse ring around it and a lone point: "both" hands the statistical stage only the radius stage's
    survivors, and a removed row keeps the first status that applied."""
    rng = np.random.RandomState(5)
    blob = (0.01 * rng.standard_normal((200, 3))).astype(np.float32)
    pair = np.array([[1.0, 0, 0], [1.005, 0, 0]], dtype=np.float32)
    cloud = np.concatenate([blob, pair, np.full((1, 3), np.nan, dtype=np.float32)])
    rad = ref.filter_cloud(cloud, "radius", radius=0.02, min_neighbours=4)
    both = ref.filter_cloud(cloud, "both", radius=0.02, min_neighbours=4, knn=5, max_radius=0.02, std_ratio=1.0)
    stat = ref.filter_cloud(cloud, "statistical", knn=1, max_radius=0.02, std_ratio=1.0)
    assert rad["status"][200:].tolist() == [1, 1, 0] and both["status"][200:].tolist() == [1, 1, 0]
    assert stat["found"][200:].tolist() == [1, 1, -1]        # the pair finds itself without the radius stage
    assert (both["found"][~rad["keep"]] == -1).all() and (both["status"][~rad["keep"]] == rad["status"][~rad["keep"]]).all()
    again = ref.knn_mean_distance(cloud, rad["keep"], 5, 0.02)
    assert again[0].tobytes() == both["mean_dist"].tobytes() and np.array_equal(again[1], both["found"])
    assert set(np.unique(both["status"])) >= {0, 1, 3, 4} and both["num"].sum() == len(cloud)
    assert np.array_equal(both["keep"], both["status"] == ref.KEPT)
    xyz, rgb = ref.apply(both["keep"], cloud, np.ones_like(cloud))
    assert (xyz[~both["keep"]].view(np.uint32) == ref.QNAN_BITS).all() and (rgb[~both["keep"]] == 0).all()
    assert xyz[both["keep"]].tobytes() == cloud[both["keep"]].tobytes() and (rgb[both["keep"]] == 1).all()


def test_against_scipys_kd_tree():
    spatial = pytest.importorskip("scipy.spatial")
    rng = np.random.RandomState(7)
    pts = rng.uniform(0.0, 0.3, size=(1500, 3)).astype(np.float32)
    tree = spatial.cKDTree(pts.astype(np.float64))
    # (radii between two float32 d2 values: no pair sits within rounding of the threshold in this seeded cloud)
    R, k = 0.04, 20
    d2_all = np.concatenate([d for _, d in ref._blocks(pts, None, 10.0)])
    assert np.abs(np.sqrt(d2_all[np.isfinite(d2_all)].astype(np.float64)) - float(f32(R))).min() > 1e-7
    n_ball = np.array([len(v) - 1 for v in tree.query_ball_point(pts.astype(np.float64), float(f32(R)))])
    assert np.array_equal(ref.radius_count(pts, None, R, 10 ** 6), n_ball)
    assert np.array_equal(ref.radius_count(pts, None, R, 16), np.minimum(n_ball, 16))
    dist, _ = tree.query(pts.astype(np.float64), k=k + 1, distance_upper_bound=float(f32(R)))
    mean, found = ref.knn_mean_distance(pts, None, k, R)
    assert np.array_equal(found, np.minimum(n_ball, k))
    full = found == k
    want = dist[full, 1:].mean(axis=1)
    # float32 rounding of a float64 evaluation: d2 carries <= 3 roundings and the root one (2.5 ulp of the distance), the mean one
    assert full.sum() > 100 and np.abs(mean[full].astype(np.float64) - want).max() <= 4 * 2.0 ** -24 * want.max()
    assert np.isnan(mean[~full]).all()


def test_the_scene_loses_every_planted_row_and_no_interior_row():
    xyz, planted, interior = ref.scene()
    assert xyz.shape == (ref.SCENE_W * ref.SCENE_H + 12, 3) and planted.sum() == 12
    surface = ref.graph_rows(xyz) & ~planted
    d2 = ref.d2_block(xyz[planted], xyz[ref.graph_rows(xyz)])
    d2[np.arange(12), np.flatnonzero(planted[ref.graph_rows(xyz)])] = np.inf
    assert np.sqrt(d2.min()) >= 2 * 0.04                      # planted >= 2 radius from every surface point and from each other
    out = ref.scene_result("radius")
    assert not out["keep"][planted].any() and (out["status"][planted] == ref.TOO_FEW_IN_RADIUS).all()
    assert interior.sum() > 5000 and out["keep"][interior].all()
    print("radius filter: %.2f %% of the surface rows removed" % (100.0 * (~out["keep"][surface]).mean()))
    both = ref.scene_result("both")
    assert not both["keep"][planted].any()
    print("both: %.2f %% of the surface rows removed" % (100.0 * (~both["keep"][surface]).mean()))
