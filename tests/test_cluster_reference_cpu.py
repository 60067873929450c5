"""tests/cluster_reference.py, the numpy restatement of the object-segmentation contract, against hand-built cases whose
answer is known by construction, and against scipy where every pair is well away from the threshold.  No GPU."""
import numpy as np
import pytest

from . import cluster_reference as ref

f32 = np.float32


def _partition(root):
    return sorted(tuple(np.nonzero(root == r)[0]) for r in np.unique(root[root >= 0]))


def test_lattice_spacing_equal_to_the_tolerance_is_joined_and_one_ulp_more_is_not():
    pts = ref.lattice((3, 3, 2), 0.5)
    t = f32(0.5)
    assert float(t * t) == 0.25 and ref.sqdist(pts[:1], pts[1:2])[0, 0] == f32(0.25)      # d2 == T2 exactly
    out = ref.cluster_points(pts, tolerance=0.5, min_points=1, max_objects=4)
    assert (out["root"] == 0).all() and tuple(out["num"]) == (1, 1) and out["size"][0] == 18
    assert out["bbox"][0].tolist() == [0.0, 0.0, 0.0, 1.0, 1.0, 0.5]
    # tolerance 0.25 on the same lattice: nothing is joined (d2 = 0.25 > 0.0625)
    out = ref.cluster_points(pts, tolerance=0.25, min_points=1, max_objects=32)
    assert np.array_equal(out["root"], np.arange(18)) and tuple(out["num"]) == (18, 18)
    # two points one ulp further apart than the tolerance
    above = np.nextafter(t, f32(1.0))
    assert f32(above * above) > f32(t * t)
    for axis in range(3):
        pair = np.zeros((2, 3), dtype=np.float32)
        pair[1, axis] = t
        assert ref.cluster_points(pair, tolerance=0.5, min_points=1)["root"].tolist() == [0, 0]
        pair[1, axis] = above
        assert ref.cluster_points(pair, tolerance=0.5, min_points=1)["root"].tolist() == [0, 1]


def _three_groups():
    """Rows 0-2 one group (size 3), 3-4 (size 2), 5-7 (size 3), 8 alone; groups 10 apart, members 0.25 apart."""
    pts = np.zeros((9, 3), dtype=np.float32)
    for rows, x in (((0, 1, 2), 0.0), ((3, 4), 10.0), ((5, 6, 7), 20.0), ((8,), 30.0)):
        for k, r in enumerate(rows):
            pts[r] = (x, 0.25 * k, 0.0)
    return pts


def test_size_ties_are_broken_by_root_and_min_points_and_max_objects_cut_where_they_should():
    pts = _three_groups()
    out = ref.cluster_points(pts, tolerance=0.25, min_points=1, max_objects=8)
    assert out["root"].tolist() == [0, 0, 0, 3, 3, 5, 5, 5, 8]
    assert out["label"].tolist() == [0, 0, 0, 2, 2, 1, 1, 1, 3]                   # sizes 3, 3, 2, 1: the tie goes to root 0
    assert out["size"][:4].tolist() == [3, 3, 2, 1] and out["first"][:4].tolist() == [0, 5, 3, 8]
    assert (out["size"][4:] == -1).all() and (out["first"][4:] == -1).all() and np.isnan(out["bbox"][4:]).all()
    assert out["bbox"][1].tolist() == [20.0, 0.0, 0.0, 20.0, 0.5, 0.0]
    for min_points, kept in ((1, 4), (2, 3), (3, 2), (4, 0)):                     # at size, size - 1 and size + 1
        assert ref.cluster_points(pts, tolerance=0.25, min_points=min_points, max_objects=8)["num"].tolist() == [kept, kept]
    for max_objects, count in ((3, 3), (4, 4), (5, 4)):                           # below, at and above the kept count
        out = ref.cluster_points(pts, tolerance=0.25, min_points=1, max_objects=max_objects)
        assert out["num"].tolist() == [count, 4] and len(out["size"]) == max_objects
        assert (out["label"] == 3).sum() == (1 if max_objects >= 4 else 0)
    out = ref.cluster_points(pts, tolerance=0.25, min_points=3, max_objects=8)
    assert out["label"].tolist() == [0, 0, 0, -1, -1, 1, 1, 1, -1] and out["root"][3] == 3    # dropped: a root but no label


def test_a_masked_bridge_splits_a_component_and_excluded_rows_have_no_root():
    pts = np.array([[0, 0, 0], [0.25, 0, 0], [0.5, 0, 0], [np.nan, 0, 0], [0.75, np.inf, 0]], dtype=np.float32)
    assert ref.cluster_points(pts, tolerance=0.25, min_points=1)["root"].tolist() == [0, 0, 0, -1, -1]
    mask = np.array([1, 0, 1, 1, 1], dtype=np.uint8)
    out = ref.cluster_points(pts, mask, tolerance=0.25, min_points=1)
    assert out["root"].tolist() == [0, -1, 2, -1, -1] and out["label"].tolist() == [0, -1, 1, -1, -1]
    empty = ref.cluster_points(np.zeros((0, 3), dtype=np.float32), max_objects=3)
    assert empty["num"].tolist() == [0, 0] and empty["size"].tolist() == [-1] * 3 and np.isnan(empty["bbox"]).all()


def test_duplicate_points_and_signed_zero_in_the_box():
    pts = np.array([[1, 1, 1]] * 4 + [[2, 2, 2]] * 2 + [[0.0, 0, 0], [-0.0, 0, 0]], dtype=np.float32)
    out = ref.cluster_points(pts, tolerance=0.125, min_points=2, max_objects=4)
    assert out["root"].tolist() == [0, 0, 0, 0, 4, 4, 6, 6] and out["size"][:3].tolist() == [4, 2, 2]
    assert out["first"][:3].tolist() == [0, 4, 6]
    box = out["bbox"][2]
    assert np.signbit(box[0]) and not np.signbit(box[3])                         # min x = -0.0, max x = +0.0


def test_assign_and_the_mask_and_the_selection():
    xyz = np.array([[0, 0, 0], [1, 0, 0], [1, 0, 0], [3, 0, 0]], dtype=np.float32)
    label = np.array([-1, 1, 0, 2], dtype=np.int32)
    r = f32(0.5)
    above = np.nextafter(r, f32(1.0))
    assert f32(above * above) > f32(r * r)
    edge = np.array([[r, 0, 0], [above, 0, 0], [0, -r, 0], [0, 0, -above]], dtype=np.float32)
    obj, point = ref.assign(edge, np.zeros((1, 3), dtype=np.float32), np.array([7], dtype=np.int32), 0.5)
    assert point.tolist() == [0, -1, 0, -1] and obj.tolist() == [7, -1, 7, -1]               # exactly R: in; one ulp more: out
    query = np.array([[1.5, 0, 0], [0.125, 0, 0], [np.nan, 0, 0], [2, 0, 0]], dtype=np.float32)
    obj, point = ref.assign(query, xyz, label, 0.5)
    assert point.tolist() == [1, -1, -1, -1] and obj.tolist() == [1, -1, -1, -1]             # equal d2: the lower row
    obj, point = ref.assign(query, xyz, label, 1.0)
    assert point.tolist() == [1, 1, -1, 1]                   # the nearest row of query 1 is unlabelled: the farther one is taken
    assert ref.assign(query[:0], xyz, label, 1.0)[0].shape == (0,)
    assert ref.assign(query, xyz[:0], label[:0], 1.0)[1].tolist() == [-1] * 4
    z = np.array([0.75, 0.76, np.nextafter(f32(f32(0.75) + f32(0.01)), f32(1.0)), 0.9], dtype=np.float32)
    pts = np.stack([np.zeros(4, np.float32), np.zeros(4, np.float32), z], axis=1)
    assert ref.above_table_mask(pts, 0.75, 0.01).tolist() == [False, bool(z[1] > f32(f32(0.75) + f32(0.01))), True, True]
    keep = [4, 0, 3, 1, 5]
    index, objects = ref.select_per_object(keep, [0, 1, 9, 0, -1, 0], 2, 2)
    assert index.tolist() == [0, 3, 1] and objects.tolist() == [0, 0, 1]
    index, objects = ref.select_per_object(keep, [0, 1, 9, 0, -1, 0], 2, 1)
    assert index.tolist() == [0, 1] and objects.tolist() == [0, 1]


@pytest.mark.parametrize("seed, n", [(1, 300), (2, 1500)])
def test_partition_agrees_with_scipy_away_from_the_threshold(seed, n):
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    from scipy.spatial import cKDTree
    pts = ref.blobs(seed, n)
    tolerance = 0.01
    d = np.sqrt(((pts[:, None].astype(np.float64) - pts[None].astype(np.float64)) ** 2).sum(-1))
    # no pair near the threshold: the float32 d2 of such a pair is within a few 2^-24 of 1e-4, 1e-9 in the distance
    assert (np.abs(d - tolerance) > 1e-8).all()
    pairs = cKDTree(pts.astype(np.float64)).query_pairs(tolerance, output_type="ndarray")
    graph = coo_matrix((np.ones(len(pairs)), (pairs[:, 0], pairs[:, 1])), shape=(n, n))
    _, comp = connected_components(graph, directed=False)
    want = sorted(tuple(np.nonzero(comp == c)[0]) for c in np.unique(comp))
    out = ref.cluster_points(pts, tolerance=tolerance, min_points=1, max_objects=n)
    assert _partition(out["root"]) == want
    sizes = out["size"][:out["num"][0]]
    assert (np.diff(sizes) <= 0).all() and sizes.sum() == n
    for r in np.unique(out["root"]):
        assert r == np.nonzero(out["root"] == r)[0].min()
