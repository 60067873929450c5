"""csrc/mesh_simplify.hip on the device against the plain-loop restatement (tests/mesh_simplify_reference.py), bit for bit: the new
vertices, their weights, the index buffer, the twelve counters and the surface's four.  The meshes are built by hand, a few
thousand rows at most, and every case runs twice for equal bytes; then ``Volume.extract_mesh().simplify()`` on a fused sphere."""
import itertools

import numpy as np
import pytest
import torch

from . import mesh_simplify_reference as sref
from . import tsdf_mesh_reference as mref
from . import tsdf_reference as ref
from .test_mesh_simplify_reference_cpu import scene_params, scene_views

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
f32 = np.float32
OUTPUTS = ("xyz", "normal", "rgb", "weight", "tri", "num", "surface_num")
ORIGIN = (0.25, -0.5, 1.0)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


class Buffers:
    """Outputs between two guard bands of 7s, so a write beyond a buffer shows."""
    GUARD = 16

    def __init__(self, mv, mt):
        g = self.GUARD
        self.store = {name: torch.full((n + 2 * g * width,), 7, dtype=dtype, device=DEV) for name, n, width, dtype in (
            ("xyz", mv * 3, 3, torch.float32), ("normal", mv * 3, 3, torch.float32), ("rgb", mv * 3, 3, torch.float32),
            ("weight", mv, 1, torch.int32), ("tri", mt * 3, 3, torch.int32), ("num", 12, 1, torch.int32),
            ("surface_num", 4, 1, torch.int32))}
        self.width = {"xyz": 3, "normal": 3, "rgb": 3, "weight": 1, "tri": 3, "num": 1, "surface_num": 1}

    def view(self, name):
        g = self.GUARD * self.width[name]
        return self.store[name][g:self.store[name].numel() - g]

    def guards_untouched(self):
        for name, t in self.store.items():
            g = self.GUARD * self.width[name]
            if not ((t[:g] == 7).all() and (t[t.numel() - g:] == 7).all()):
                return False
        return True


def _launch(L, xyz, normal, rgb, num, tri, num_tri, origin, cell, grid, dedupe, mv, mt, buffers, stream=None):
    from regnet_for_3d_grasping_amd import _lib
    rows, mt_in = int(xyz.shape[0]), int(tri.shape[0])
    cells = grid[0] * grid[1] * grid[2]
    workspace = torch.empty((int(L.regnet_mesh_simplify_workspace_bytes(cells, mt_in)) // 8,), dtype=torch.int64, device=DEV)
    o = np.ascontiguousarray(np.asarray(origin, dtype=np.float64).astype(np.float32))
    v = buffers.view
    _lib.call("regnet_mesh_simplify_f32", xyz, xyz.data_ptr(), normal.data_ptr(), rgb.data_ptr(), rows, num.data_ptr(),
              tri.data_ptr(), mt_in, num_tri.data_ptr(), o.ctypes.data, float(cell), grid[0], grid[1], grid[2], int(dedupe), mv, mt,
              workspace.data_ptr(), v("xyz").data_ptr(), v("normal").data_ptr(), v("rgb").data_ptr(), v("weight").data_ptr(),
              v("tri").data_ptr(), v("num").data_ptr(), v("surface_num").data_ptr(),
              stream=None if stream is None else stream.cuda_stream)
    return workspace


def _check(xyz, normal, rgb, tri, grid, cell=0.3, dedupe=1, K=None, Kt=None, mv=None, mt=None, origin=ORIGIN, stream=None):
    """The device twice against the restatement, every output byte for byte -> the restatement's dict."""
    from regnet_for_3d_grasping_amd import _lib
    xyz, normal, rgb = (np.ascontiguousarray(np.asarray(a, dtype=np.float32).reshape(-1, 3)) for a in (xyz, normal, rgb))
    tri = np.ascontiguousarray(np.asarray(tri, dtype=np.int32).reshape(-1, 3))
    K = len(xyz) if K is None else K
    Kt = len(tri) if Kt is None else Kt
    mv = max(len(xyz), 1) if mv is None else mv
    mt = max(len(tri), 1) if mt is None else mt
    want = sref.simplify(xyz, normal, rgb, K, tri, Kt, origin, cell, grid, dedupe, mv, mt)
    pad = lambda a, dtype: a if len(a) else np.zeros((1, 3), dtype=dtype)      # noqa: E731  (a capacity is at least 1)
    d = [_dev(pad(xyz, np.float32)), _dev(pad(normal, np.float32)), _dev(pad(rgb, np.float32)),
         _dev(np.array([K, K, 0, 0], dtype=np.int32)), _dev(pad(tri, np.int32)), _dev(np.array([Kt, Kt, 0, 0], dtype=np.int32))]
    ctx = torch.cuda.stream(stream) if stream is not None else torch.cuda.device(DEV)
    with ctx:
        for _ in range(2):
            buffers = Buffers(mv, mt)
            if stream is not None:
                torch.cuda.synchronize()
            keep = _launch(_lib.lib, *d, origin, cell, grid, dedupe, mv, mt, buffers, stream=stream)
            torch.cuda.synchronize()
            del keep
            for name in OUTPUTS:
                got = buffers.view(name).cpu().numpy()
                assert got.tobytes() == want[name].tobytes(), (name, got.reshape(want[name].shape)[:8], want[name][:8])
            assert buffers.guards_untouched()
    return want


def _at(cell_index, fraction=(0.5, 0.5, 0.5), cell=0.3, origin=ORIGIN):
    """A point in cell ``(ix, iy, iz)`` at ``fraction`` of its edges, float32."""
    return [f32(origin[k] + (cell_index[k] + fraction[k]) * cell) for k in range(3)]


def _unit(rng, n):
    v = rng.normal(size=(n, 3))
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)


def _random_mesh(rng, grid, n_vertices, n_triangles, cell=0.3, spread=0.0):
    """Vertices uniform over the grid's box (``spread`` cells beyond it on every side) and random triangles."""
    g = np.asarray(grid, dtype=np.float64)
    xyz = (np.asarray(ORIGIN) + rng.uniform(-spread, g + spread, size=(n_vertices, 3)) * cell).astype(np.float32)
    tri = rng.randint(0, n_vertices, size=(n_triangles, 3)).astype(np.int32)
    return xyz, _unit(rng, n_vertices), rng.uniform(-0.1, 1.1, size=(n_vertices, 3)).astype(np.float32), tri


def test_a_vertex_on_a_cell_face_and_one_ulp_either_side():
    grid = (4, 3, 2)
    face = f32(ORIGIN[0] + 2 * 0.3)
    below, above = np.nextafter(face, f32(-9)), np.nextafter(face, f32(9))
    xs = [f32(face - 8 * (face - below)), below, face, above, f32(face + 8 * (above - face))]
    xyz = [[x, _at((0, 1, 0))[1], _at((0, 0, 1))[2]] for x in xs] + [_at((0, 0, 0)), _at((3, 2, 1))]
    tri = [[i, 5, 6] for i in range(5)]
    out = _check(xyz, _unit(np.random.RandomState(1), 7), np.full((7, 3), 0.5), tri, grid)
    cells = out["vertex_cell"][:5] % 4
    assert cells.tolist() == sorted(cells.tolist()) and cells[0] == 1 and cells[4] == 2      # the face separates them
    # ... and on the grid's own faces: the low one is inside, the high one is not
    lo, hi = f32(ORIGIN[0]), f32(ORIGIN[0] + 4 * 0.3)
    xyz = [[x, _at((0, 1, 0))[1], _at((0, 0, 1))[2]] for x in (np.nextafter(lo, f32(-9)), lo, np.nextafter(hi, f32(-9)), hi,
                                                                np.nextafter(hi, f32(9)))] + [_at((1, 0, 0)), _at((2, 2, 1))]
    out = _check(xyz, _unit(np.random.RandomState(2), 7), np.full((7, 3), 0.5), [[i, 5, 6] for i in range(5)], grid)
    assert (out["vertex_cell"][:5] >= 0).tolist() == [False, True, True, out["vertex_cell"][3] >= 0, False]
    assert out["num"][4] >= 2 and out["num"][11] == out["num"][4]


def test_a_lone_vertex_is_kept_bit_for_bit():
    """Out-of-range colours, a NaN with a payload in the normal, an unnormalised normal: the cell's one row as it was given."""
    grid = (3, 3, 3)
    xyz = np.array([_at((0, 0, 0), (0.123, 0.987, 0.5)), _at((1, 2, 0), (0.3, 0.3, 0.3)), _at((2, 1, 2), (0.9, 0.01, 0.7))], dtype=np.float32)
    normal = np.array([[0.1, 7.0, -3.0], [0, 0, 0], [1, 0, 0]], dtype=np.float32)
    normal[1] = np.array([0x7fc12345, 0xffc00001, 0x7f800000], dtype=np.uint32).view(np.float32)
    rgb = np.array([[1.5, -0.25, 0.3], [np.nan, 0.1, 0.2], [0, 1, 0.5]], dtype=np.float32)
    out = _check(xyz, normal, rgb, [[2, 1, 0]], grid)
    order = np.argsort(out["vertex_cell"])
    for name, source in (("xyz", xyz), ("normal", normal), ("rgb", rgb)):
        assert out[name][:3].tobytes() == source[order].tobytes(), name
    assert out["weight"][:3].tolist() == [1, 1, 1] and out["num"][0] == 3


def test_five_thousand_vertices_contend_for_one_cell():
    rng = np.random.RandomState(5)
    grid = (5, 4, 3)
    busy = np.array([_at((2, 1, 1), rng.uniform(0.001, 0.999, size=3)) for _ in range(5000)], dtype=np.float32)
    xyz = np.concatenate([busy, np.array([_at((0, 0, 0)), _at((4, 3, 2))], dtype=np.float32)])
    normal = _unit(rng, 5002)
    normal[:5000] = (normal[:5000] + np.array([0, 0, 2.0], dtype=np.float32))
    normal /= np.linalg.norm(normal, axis=1, keepdims=True)
    tri = [[int(rng.randint(5000)), 5000, 5001] for _ in range(64)]
    out = _check(xyz, normal, rng.uniform(size=(5002, 3)), tri, grid)
    assert sorted(out["weight"][:3].tolist()) == [1, 1, 5000] and out["num"][6] == 1 and out["num"][10] == 63


def test_duplicates_rotations_the_smallest_row_and_the_opposite_orientation():
    """Cells a < b < c.  Rows of the three rotations of (a, b, c) are one triangle; (a, c, b) and its rotations another; the
    survivor is the smallest source row although the copies sit in different workgroups between 3000 other rows."""
    rng = np.random.RandomState(6)
    grid = (6, 5, 4)
    xyz, normal, rgb, tri = _random_mesh(rng, grid, 400, 3000)
    corner = [0, 1, 2]                                          # three vertices in three known cells
    xyz[0], xyz[1], xyz[2] = _at((0, 0, 0)), _at((3, 2, 1)), _at((5, 4, 3))
    tri[(tri < 3)] += 3                                         # no other row uses them
    rows = rng.permutation(3000)[:40]
    for j, t in enumerate(rows[:24]):
        tri[t] = np.roll(corner, j % 3)
    for j, t in enumerate(rows[24:]):
        tri[t] = np.roll(corner[::-1], j % 3)
    out = _check(xyz, normal, rgb, tri, grid)
    a, b, c = (int(np.nonzero(out["cells"] == out["vertex_cell"][v])[0][0]) for v in corner)
    kept = out["tri"][:int(out["num"][5])]
    forward = np.nonzero((kept == [a, b, c]).all(axis=1))[0]
    backward = np.nonzero((kept == [a, c, b]).all(axis=1))[0]
    assert len(forward) == 1 and len(backward) == 1
    assert out["source"][forward[0]] == rows[:24].min() and out["source"][backward[0]] == rows[24:].min()
    assert out["num"][10] >= 38
    without = _check(xyz, normal, rgb, tri, grid, dedupe=0)
    assert without["num"][10] == 0 and without["num"][6] == out["num"][6] + out["num"][10]


def test_keys_planted_on_one_home_slot_and_a_probe_that_wraps():
    """12 source rows: a table of 32 slots.  Six different triples whose home is the LAST slot, each twice: the probes run over the
    table's end, and every key still finds its own slot."""
    from regnet_for_3d_grasping_amd import _lib
    L = _lib.lib
    grid = (6, 5, 4)
    assert L.regnet_mesh_simplify_table_slots(12) == 32
    planted = []
    for c in itertools.permutations(range(120), 3):
        if c[0] < c[1] and c[0] < c[2] and L.regnet_mesh_simplify_home_slot_host(c[0] << 42 | c[1] << 21 | c[2], 32) == 31:
            planted.append(c)
            if len(planted) == 6:
                break
    assert len(planted) == 6
    xyz = np.array([_at((c % 6, c // 6 % 5, c // 30)) for c in range(120)], dtype=np.float32)      # vertex c in cell c
    tri = [list(np.roll(c, j)) for j in (0, 1) for c in planted]
    out = _check(xyz, _unit(np.random.RandomState(7), 120), np.full((120, 3), 0.25), tri, grid)
    assert out["vertex_cell"].tolist() == list(range(120))
    assert out["num"][6] == 6 and out["num"][10] == 6 and out["source"].tolist() == [0, 1, 2, 3, 4, 5]


def test_collapsed_stray_and_absent_rows_and_a_cell_that_is_not_emitted():
    grid = (4, 4, 4)
    nan = np.nan
    xyz = [_at((0, 0, 0)), _at((0, 0, 0), (0.1, 0.2, 0.3)), _at((0, 0, 0), (0.9, 0.9, 0.9)),      # 0-2: one cell
           _at((1, 1, 1)), _at((2, 2, 2)), _at((3, 3, 3)),                                         # 3-5: three cells
           _at((1, 2, 3)), _at((1, 2, 3), (0.2, 0.2, 0.2)),                                        # 6-7: a cell that only collapses
           [nan, 0.0, 1.2], [0.5, np.inf, 1.2],                                                    # 8-9: not finite
           _at((-1, 0, 0)), _at((4, 0, 0)), _at((0, -1, 0)), _at((0, 4, 0)), _at((0, 0, -1)), _at((0, 0, 4)),      # 10-15: outside
           _at((3, 0, 0))]                                                                         # 16: never referenced
    tri = [[3, 4, 5], [0, 1, 3], [0, 1, 2], [6, 7, 3], [6, 6, 6],       # kept, 2 equal, 3 equal, 2 equal, 3 equal
           [-1, -1, -1], [3, 4, 8], [9, 4, 5], [3, 4, 17], [3, -2, 5], [-1, 4, 5], [1 << 30, 4, 5]] + [[3, 4, v] for v in range(10, 16)]
    out = _check(xyz, _unit(np.random.RandomState(8), 17), np.full((17, 3), 0.75), tri, grid)
    assert out["num"].tolist() == [3, 3, 0, 6, 8, 1, 1, 0, 0, 4, 0, 13]
    assert out["tri"][0].tolist() == [0, 1, 2] and out["weight"][:3].tolist() == [1, 1, 1]
    assert out["vertex_cell"][6] not in out["cells"]            # occupied, referenced by collapsed rows only: not emitted


def test_normals_that_are_nan_and_normals_that_cancel():
    grid = (4, 4, 4)
    xyz = [_at((0, 0, 0), (0.2, 0.2, 0.2)), _at((0, 0, 0), (0.6, 0.6, 0.6)),       # two NaN normals: ncount == 0
           _at((1, 1, 1), (0.2, 0.2, 0.2)), _at((1, 1, 1), (0.6, 0.6, 0.6)),       # n and -n: len == 0
           _at((2, 2, 2), (0.2, 0.2, 0.2)), _at((2, 2, 2), (0.6, 0.6, 0.6)),       # one NaN, one finite: the finite one
           _at((3, 3, 3), (0.2, 0.2, 0.2)), _at((3, 3, 3), (0.6, 0.6, 0.6))]       # one with a single infinite component
    n = np.array([0.6, -0.8, 0.0], dtype=np.float32)
    normal = [[np.nan] * 3, [np.nan, 0, 1], n, -n, [np.nan] * 3, n, [np.inf, 0, 0], [0, 0, -1]]
    out = _check(xyz, normal, np.full((8, 3), 0.5), [[0, 2, 4], [1, 3, 6], [5, 7, 0]], grid)
    got = out["normal"][:4]
    assert np.isnan(got[0]).all() and np.isnan(got[1]).all()
    assert np.allclose(got[2], n, atol=1e-6) and got[3].tolist() == [0.0, 0.0, -1.0] and out["weight"][:4].tolist() == [2, 2, 2, 2]


@pytest.mark.parametrize("grid,rows", [((1, 1, 1), (300, 500)), ((7, 3, 5), (1500, 4000)), ((1, 64, 1), (700, 2100)),
                                       ((33, 2, 31), (3000, 2900))])
@pytest.mark.parametrize("dedupe", [0, 1])
def test_grids_with_random_meshes(grid, rows, dedupe):
    """Vertices up to half a cell beyond the grid, a NaN row, rows of -1, indices beyond K: more than one workgroup of every
    kernel, block counts that are no multiple of anything."""
    rng = np.random.RandomState(sum(grid) + dedupe)
    xyz, normal, rgb, tri = _random_mesh(rng, grid, rows[0], rows[1], spread=0.5)
    xyz[rng.randint(rows[0], size=5)] = np.nan
    normal[rng.randint(rows[0], size=20), rng.randint(3, size=20)] = np.nan
    tri[rng.randint(rows[1], size=30)] = -1
    tri[rng.randint(rows[1], size=30), rng.randint(3, size=30)] = rows[0] - 3      # beyond K = rows - 7
    out = _check(xyz, normal, rgb, tri, grid, dedupe=dedupe, K=rows[0] - 7, Kt=rows[1] - 11)
    assert out["num"][6] + out["num"][9] + out["num"][10] + out["num"][11] == rows[1] - 11
    if grid == (1, 1, 1):
        assert out["num"][:2].tolist() == [0, 0] and out["num"][3] == 1 and out["num"][6] == 0 and out["num"][9] > 0
    else:
        assert out["num"][0] > 0 and out["num"][6] > 0 and out["num"][4] > 0


def test_both_capacities_keep_the_smallest_cells_and_source_rows():
    rng = np.random.RandomState(11)
    grid = (7, 3, 5)
    xyz, normal, rgb, tri = _random_mesh(rng, grid, 1500, 4000)
    full = _check(xyz, normal, rgb, tri, grid)
    kv, kt = int(full["num"][1]), int(full["num"][6])
    mv, mt = kv // 2, kt // 3
    few = _check(xyz, normal, rgb, tri, grid, mv=mv, mt=mt)      # (the guards beyond both buffers are checked there)
    lost = (full["tri"][:mt] >= mv).any(axis=1)
    assert few["num"].tolist() == [mv, kv, 1, full["num"][3], full["num"][4], mt, kt, int(lost.sum()), 1] + full["num"][9:].tolist()
    assert 0 < lost.sum() < mt and few["surface_num"].tolist() == [mv, kv, 1500, 1]
    assert few["xyz"].tobytes() == full["xyz"][:mv].tobytes() and (few["tri"][lost] == -1).all()
    assert np.array_equal(few["tri"][~lost], full["tri"][:mt][~lost])
    one = _check(xyz, normal, rgb, tri, grid, mv=1, mt=1)
    assert one["num"][:3].tolist() == [1, kv, 1] and one["num"][5:9].tolist() == [1, kt, 1, 1]


@pytest.mark.parametrize("dedupe", [0, 1])
def test_empty_meshes(dedupe):
    rng = np.random.RandomState(12)
    grid = (3, 3, 3)
    xyz, normal, rgb, tri = _random_mesh(rng, grid, 50, 80)
    for K, Kt in ((0, 80), (50, 0), (0, 0)):
        out = _check(xyz, normal, rgb, tri, grid, dedupe=dedupe, K=K, Kt=Kt, mv=9, mt=5)
        assert out["num"].tolist() == [0, 0, 0, out["num"][3], out["num"][4], 0, 0, 0, 0, 0, 0, Kt if K == 0 else 0]
        assert (out["tri"] == -1).all() and (out["weight"] == -1).all() and np.isnan(out["xyz"]).all()


def test_side_stream():
    rng = np.random.RandomState(13)
    grid = (7, 3, 5)
    stream = torch.cuda.Stream(device=DEV)
    out = _check(*_random_mesh(rng, grid, 900, 2000), grid, stream=stream)
    assert out["num"][6] > 0


def test_simplify_replays_from_a_graph():
    """Two fills and eight launches: the replay follows the mesh as it then stands, K and Kt included."""
    from regnet_for_3d_grasping_amd import _lib
    grid = (7, 3, 5)
    mv, mt = 1200, 2500
    rng = np.random.RandomState(14)
    d = [torch.zeros((1200, 3), dtype=torch.float32, device=DEV) for _ in range(3)]
    num, num_tri = torch.zeros((4,), dtype=torch.int32, device=DEV), torch.zeros((4,), dtype=torch.int32, device=DEV)
    tri = torch.zeros((2500, 3), dtype=torch.int32, device=DEV)
    buffers = Buffers(mv, mt)
    side = torch.cuda.Stream(device=DEV)
    with torch.cuda.stream(side):
        _launch(_lib.lib, *d, num, tri, num_tri, ORIGIN, 0.3, grid, 1, mv, mt, buffers)
    side.synchronize()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        keep = _launch(_lib.lib, *d, num, tri, num_tri, ORIGIN, 0.3, grid, 1, mv, mt, buffers)
    for K, Kt in ((1200, 2500), (700, 1900)):
        xyz, normal, rgb, t = _random_mesh(rng, grid, 1200, 2500)
        t[t >= K] = K - 1
        for dst, src in zip(d + [tri], (xyz, normal, rgb, t)):
            dst.copy_(_dev(src))
        num.copy_(_dev(np.array([K, K, 0, 0], dtype=np.int32)))
        num_tri.copy_(_dev(np.array([Kt, Kt, 0, 0], dtype=np.int32)))
        graph.replay()
        torch.cuda.synchronize()
        want = sref.simplify(xyz, normal, rgb, K, t, Kt, ORIGIN, 0.3, grid, 1, mv, mt)
        for name in OUTPUTS:
            assert buffers.view(name).cpu().numpy().tobytes() == want[name].tobytes(), name
    assert buffers.guards_untouched()
    del keep


def test_every_error_code():
    from regnet_for_3d_grasping_amd import _lib
    L = _lib.lib
    SHAPE, NULL, UNSUPPORTED = -1, -2, -3
    buf = torch.zeros((1 << 16,), dtype=torch.float32, device=DEV)
    p = buf.data_ptr()
    before = buf.clone()
    origin = np.zeros(3, dtype=np.float32)
    names = ("xyz", "normal", "rgb", "K_source", "tri", "num_tri_in", "origin3", "workspace", "out_xyz", "out_normal", "out_rgb",
             "out_weight", "out_tri", "num")

    def call(rows=8, max_tri_in=8, cell=0.5, grid=(2, 2, 2), dedupe=1, max_vertices=8, max_triangles=8, **null):
        a = {name: (origin.ctypes.data if name == "origin3" else p) for name in names + ("surface_num",)}
        a.update(null)
        return L.regnet_mesh_simplify_f32(a["xyz"], a["normal"], a["rgb"], rows, a["K_source"], a["tri"], max_tri_in, a["num_tri_in"],
                                          a["origin3"], cell, *grid, dedupe, max_vertices, max_triangles, a["workspace"],
                                          a["out_xyz"], a["out_normal"], a["out_rgb"], a["out_weight"], a["out_tri"], a["num"],
                                          a["surface_num"], None)
    for bad in (dict(rows=0), dict(max_tri_in=0), dict(grid=(0, 2, 2)), dict(grid=(2, -1, 2)), dict(grid=(2, 2, 0)), dict(dedupe=2),
                dict(dedupe=-1), dict(max_vertices=0), dict(max_triangles=0)):
        assert call(**bad) == SHAPE, bad
    for bad in (dict(grid=(1 << 11, 1 << 10, 2)), dict(grid=(1 << 40, 1 << 40, 1 << 40)), dict(max_vertices=(1 << 21) + 1),
                dict(max_triangles=(1 << 22) + 1), dict(max_tri_in=(1 << 22) + 1), dict(cell=0.0), dict(cell=-1.0),
                dict(cell=float("nan")), dict(cell=float("inf")), dict(cell=1e-60), dict(cell=1e60), dict(workspace=p + 4)):
        assert call(**bad) == UNSUPPORTED, bad
    for name in names:
        assert call(**{name: None}) == NULL, name
    assert L.regnet_mesh_simplify_workspace_bytes(8, 0) == -1 and L.regnet_mesh_simplify_workspace_bytes(8, 8) > 0
    torch.cuda.synchronize()
    assert torch.equal(buf, before)                           # every error was returned before any launch or fill


# ---- Volume.extract_mesh().simplify() ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sphere_volume():
    """The sphere of tests/test_mesh_simplify_reference_cpu.py integrated at 32^3 on the device and in numpy."""
    from regnet_for_3d_grasping_amd import tsdf
    params = scene_params(32, voxel=0.003)
    clouds, shapes, poses = scene_views("sphere")
    want, _, _ = ref.fuse_volume(clouds, shapes, poses, **params)
    vol = tsdf.Volume(tsdf.TsdfParams(**params), DEV)
    k = shapes[0][2]
    for (xyz, _), pose in zip(clouds, poses):
        vol.integrate((_dev(xyz), None, shapes[0][0], shapes[0][1], k), pose)
    torch.cuda.synchronize()
    assert vol.D.cpu().numpy().tobytes() == want.D.tobytes() and vol.W.cpu().numpy().tobytes() == want.W.tobytes()
    return vol, want


def _same_mesh(got, want):
    s = got.surface
    for name, t in (("xyz", s.xyz), ("normal", s.normal), ("rgb", s.rgb), ("weight", s.weight), ("tri", got.triangles),
                    ("num", got.report), ("surface_num", s.num)):
        assert t.cpu().numpy().tobytes() == want[name].tobytes(), name
    assert got.num_triangles.cpu().numpy().tolist() == want["num"][5:9].tolist()


@pytest.mark.parametrize("factor,dedupe", [(4, True), (3, True), (2, False)])
def test_extract_mesh_simplify_matches_the_restatement(sphere_volume, factor, dedupe):
    from regnet_for_3d_grasping_amd import tsdf
    vol, want = sphere_volume
    full = mref.mesh(want, 1 << 15)
    mesh = vol.extract_mesh(max_points=1 << 14, max_triangles=1 << 15)
    simple = mesh.simplify(factor=factor, dedupe=dedupe)
    cell = factor * 0.003
    grid = sref.grid_for((32, 32, 32), 0.003, cell)
    assert isinstance(simple, tsdf.SimplifiedMesh) and simple.source is mesh and simple.grid == grid and simple.cell == cell
    s = full["surface"]
    mv = min(1 << 14, grid[0] * grid[1] * grid[2])
    expected = sref.simplify(s["xyz"], s["normal"], s["rgb"], s["num"][0], full["tri"], full["num"][0], want.origin, cell, grid,
                             int(dedupe), mv, 1 << 15)
    _same_mesh(simple, expected)
    kv, kt = simple.check()
    assert (kv, kt) == (int(expected["num"][0]), int(expected["num"][5])) and 0 < kt < int(full["num"][0])
    if not dedupe:                                              # the sphere's mesh is closed: the chain stays closed
        assert sref.balanced(full["tri"][:int(full["num"][0])]) and sref.balanced(simple.to_host()[3])
    # a second call allocates nothing and writes the same tensors; out= takes an earlier result's
    again = mesh.simplify(factor=factor, dedupe=dedupe)
    assert again is simple and len(vol.simplify_buffers) >= 1
    other = tsdf.SimplifiedMesh.empty(mv, 1 << 15, mesh.surface.params, DEV)
    assert mesh.simplify(factor=factor, dedupe=dedupe, out=other) is other
    _same_mesh(other, expected)
    # ... and through extract_mesh(simplify=)
    _same_mesh(vol.extract_mesh(max_points=1 << 14, max_triangles=1 << 15, simplify=cell), sref.simplify(
        s["xyz"], s["normal"], s["rgb"], s["num"][0], full["tri"], full["num"][0], want.origin, cell, grid, 1, mv, 1 << 15))
    with pytest.raises(ValueError, match="2\\^21"):
        mesh.simplify(cell=0.0005)
    with pytest.raises(ValueError):
        mesh.simplify(cell=0.0)
    with pytest.raises(ValueError):
        mesh.simplify(max_triangles=(1 << 22) + 1)


def test_simplified_mesh_overflow_and_save_ply(sphere_volume, tmp_path):
    vol, _ = sphere_volume
    simple = vol.extract_mesh(max_points=1 << 14, max_triangles=1 << 15).simplify(factor=4)
    kv, kt = simple.check()
    vertices, normals, colours, triangles = simple.to_host()
    assert len(vertices) == kv and len(triangles) == kt and triangles.min() == 0 and triangles.max() == kv - 1
    path = tmp_path / "simple.ply"
    simple.save_ply(str(path))
    raw = path.read_bytes()
    end = raw.index(b"end_header\n") + len(b"end_header\n")
    assert b"element vertex %d\n" % kv in raw[:end] and b"element face %d\n" % kt in raw[:end] and len(raw) == end + 27 * kv + 13 * kt
    vertex = np.frombuffer(raw, dtype=[("xyz", "<f4", (3,)), ("n", "<f4", (3,)), ("rgb", "u1", (3,))], count=kv, offset=end)
    face = np.frombuffer(raw, dtype=[("n", "u1"), ("v", "<i4", (3,))], count=kt, offset=end + 27 * kv)
    assert vertex["xyz"].tobytes() == vertices.tobytes() and vertex["n"].tobytes() == normals.tobytes()
    assert np.array_equal(face["v"], triangles)
    small = vol.extract_mesh(max_points=1 << 14, max_triangles=1 << 15).simplify(factor=4, max_vertices=kv // 2, max_triangles=kt)
    with pytest.raises(ValueError, match="max_points = %d" % (kv // 2)):
        small.check()
    assert len(small.to_host()[3]) == kt - int(small.report[7].item()) < kt
