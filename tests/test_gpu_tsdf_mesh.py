"""csrc/tsdf_mesh.hip on the device against the plain-loop restatement (tests/tsdf_mesh_reference.py), bit for bit: the index
buffer, the four counters, the -1 rows in place, and the surface inside the ``Mesh`` against ``Volume.extract()`` of the same
state.  Every case runs twice for equal bytes.  The volumes are set by hand: sizes chosen to break the indexing."""
import ctypes

import numpy as np
import pytest
import torch

from . import tsdf_mesh_reference as mref
from . import tsdf_reference as ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
f32 = np.float32
SURFACE = ("xyz", "rgb", "normal", "weight", "num")


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _volumes(dims, D, Wt, C=None, **params):
    """One hand-set volume on the device and in numpy."""
    from regnet_for_3d_grasping_amd import tsdf
    params = dict(dict(voxel=0.5, trunc=1.0, origin=(0.25, -0.5, 1.0), dims=dims, max_points=1 << 14), **params)
    want = ref.Volume(**params)
    want.D = np.asarray(D, dtype=np.float32).reshape(-1).copy()
    want.W = np.asarray(Wt, dtype=np.int32).reshape(-1).copy()
    if C is not None:
        want.C = np.asarray(C, dtype=np.float32).reshape(-1, 3).copy()
    assert want.D.shape == want.W.shape == (want.n,)
    vol = tsdf.Volume(tsdf.TsdfParams(**params), DEV)
    vol.D.copy_(_dev(want.D))
    vol.W.copy_(_dev(want.W))
    vol.C.copy_(_dev(np.ascontiguousarray(want.C.T)))
    return vol, want


def _same(mesh, expected, plain=None):
    assert mesh.triangles.dtype == mesh.num_triangles.dtype == torch.int32
    got_num, got_tri = mesh.num_triangles.cpu().numpy(), mesh.triangles.cpu().numpy()
    assert np.array_equal(got_num, expected["num"]), (got_num, expected["num"])
    assert np.array_equal(got_tri, expected["tri"])
    assert (got_tri[int(expected["num"][0]):] == -1).all()
    for name in SURFACE:
        got = getattr(mesh.surface, name).cpu().numpy()
        assert got.tobytes() == expected["surface"][name].tobytes(), name
        if plain is not None:
            assert got.tobytes() == getattr(plain, name).cpu().numpy().tobytes(), name


def _check(dims, D, Wt, C=None, max_triangles=1 << 14, stream=None, out_mesh=None, **params):
    """``extract``, then ``extract_mesh`` twice, against the restatement -> (mesh, the restatement's dict)."""
    vol, want = _volumes(dims, D, Wt, C, **params)
    expected = mref.mesh(want, max_triangles)
    plain = vol.extract(stream=stream)
    first = vol.extract_mesh(max_triangles=max_triangles, stream=stream, out_mesh=out_mesh)
    second = vol.extract_mesh(max_triangles=max_triangles, stream=stream)
    if stream is not None:
        stream.synchronize()
    _same(first, expected, plain)
    _same(second, expected, plain)
    return first, expected


def _random(dims, seed, zero_share=0.04, top=1.04):
    """Distances in [-1, top) and a share of unobserved voxels: most cells are meshed, some have a corner that is not usable."""
    rng = np.random.RandomState(seed)
    n = dims[0] * dims[1] * dims[2]
    D = rng.uniform(-1, top, size=n).astype(np.float32)
    Wt = ((rng.uniform(size=n) >= zero_share) * rng.randint(1, 4, size=n)).astype(np.int32)
    return D, Wt, rng.uniform(size=(n, 3)).astype(np.float32)


@pytest.mark.parametrize("dims", [(2, 2, 2),         # one cell
                                  (65, 3, 2),        # a wave straddles rows
                                  (63, 5, 3),
                                  (17, 16, 17),      # blocks of 256 straddle layers
                                  (130, 7, 5),
                                  (1, 9, 9), (9, 1, 9), (9, 9, 1)])     # no cell: a valid empty mesh
def test_ragged_volumes(dims):
    D, Wt, C = _random(dims, sum(dims))
    if dims == (2, 2, 2):
        D, Wt = np.array([-0.5, 0.5, 0.25, -0.75, 0.5, 0.5, -0.25, 0.5], dtype=np.float32), np.ones(8, dtype=np.int32)
    _, out = _check(dims, D, Wt, C)
    if min(dims) < 2:
        assert out["num"].tolist() == [0, 0, 0, 0]
    else:
        assert out["num"][0] == out["num"][1] > 0 and out["num"][2] == 0


def test_every_case_of_the_table():
    """16 x 16 groups of 2^3 voxels, three voxels apart with an unobserved voxel between them: group (gx, gy) is one cell with the
    case gx + 16 gy, and no other cell is meshed."""
    dims = (48, 48, 2)
    D = np.full((2, 48, 48), 0.5, dtype=np.float32)           # [iz, iy, ix]
    Wt = np.zeros((2, 48, 48), dtype=np.int32)
    for case in range(256):
        x, y = 3 * (case % 16), 3 * (case // 16)
        Wt[:, y:y + 2, x:x + 2] = 1
        for c in range(8):
            if case >> c & 1:
                D[c >> 2 & 1, y + (c >> 1 & 1), x + (c & 1)] = -0.25 - 0.03125 * c
    _, out = _check(dims, D, Wt)
    cells, counts = np.unique(out["cells"], return_counts=True)
    want = {48 * 3 * (case // 16) + 3 * (case % 16): int(mref.TRIANGLES[case]) for case in range(1, 255)}
    assert dict(zip(cells.tolist(), counts.tolist())) == want and out["num"][1] == 820


def test_lookups_across_blocks_layers_faces_and_the_last_edge():
    """Every corner usable on 17 x 16 x 17 (272 voxels per layer: blocks straddle layers and rows): cells at all six faces of the
    volume, vertices owned by a voxel of the next block and of the next layer, and the volume's last edge."""
    dims = (17, 16, 17)
    n = 17 * 16 * 17
    rng = np.random.RandomState(7)
    D = rng.uniform(-1, 0.99, size=n).astype(np.float32)
    D[n - 1], D[n - 2] = -0.5, 0.5
    _, out = _check(dims, D, np.full(n, 2), max_triangles=1 << 15, max_points=1 << 15)
    cells = out["cells"]
    ix, iy, iz = cells % 17, cells // 17 % 16, cells // 272
    assert (ix == 0).any() and (ix == 15).any() and (iy == 0).any() and (iy == 14).any() and (iz == 0).any() and (iz == 15).any()
    kt = int(out["num"][0])
    owner = out["surface"]["keys"][out["tri"][:kt]] // 3      # the voxel that owns each triangle corner's edge
    assert (owner // 256 > cells[:kt, None] // 256).any() and (owner // 272 > cells[:kt, None] // 272).any()
    assert (out["surface"]["keys"][out["tri"][:kt]] == 3 * (n - 2)).any()


@pytest.mark.parametrize("min_weight", [1, 2, 3])
def test_min_weight_with_scrambled_weights(min_weight):
    dims = (21, 13, 6)
    D, _, C = _random(dims, 31)
    Wt = np.random.RandomState(32).randint(0, 5, size=21 * 13 * 6)
    Wt[np.random.RandomState(33).uniform(size=Wt.size) < 0.6] = 3
    _, out = _check(dims, D, Wt, C, min_weight=min_weight)
    assert out["num"][1] > 0


def test_a_nan_distance_is_not_usable_not_inside_and_not_an_error():
    dims = (9, 8, 7)
    D, Wt, C = _random(dims, 41, zero_share=0.0, top=0.99)
    _, whole = _check(dims, D, Wt, C)
    v = (3 * 8 + 4) * 9 + 5
    D[v] = np.nan
    _, holed = _check(dims, D, Wt, C)
    touching = {v - dx - 9 * dy - 72 * dz for dx, dy, dz in mref.CORNERS}
    assert set(holed["cells"].tolist()) == set(whole["cells"].tolist()) - touching and holed["num"][1] < whole["num"][1]


def test_capacity_keeps_the_smallest_cells_and_writes_nothing_beyond():
    dims = (17, 16, 17)
    D, Wt, C = _random(dims, 51, zero_share=0.0, top=0.99)
    _, full = _check(dims, D, Wt, C, max_triangles=1 << 15, max_points=1 << 15)
    total = int(full["num"][1])
    mt, canary = 1000, 16
    assert total > mt
    store = torch.full(((mt + 2 * canary) * 3,), 7, dtype=torch.int32, device=DEV)
    num = torch.full((4 + 2 * canary,), 7, dtype=torch.int32, device=DEV)
    out_mesh = (store[canary * 3:(canary + mt) * 3].view(mt, 3), num[canary:canary + 4])
    mesh, few = _check(dims, D, Wt, C, max_triangles=mt, max_points=1 << 15, out_mesh=out_mesh)
    assert few["num"].tolist() == [mt, total, 0, 1] and np.array_equal(few["tri"], full["tri"][:mt])
    assert (store[:canary * 3] == 7).all() and (store[(canary + mt) * 3:] == 7).all()
    assert (num[:canary] == 7).all() and (num[canary + 4:] == 7).all()
    with pytest.raises(ValueError, match="max_triangles = 1000"):
        mesh.check()


def test_a_surface_that_overflowed_drops_triangles_in_place():
    dims = (17, 16, 17)
    D, Wt, C = _random(dims, 51, zero_share=0.0, top=0.99)
    _, full = _check(dims, D, Wt, C, max_triangles=1 << 15, max_points=1 << 15)
    total, rows = int(full["num"][1]), int(full["surface"]["num"][1])
    mp, mt, canary = rows // 3, 1 << 15, 16
    store = torch.full(((mt + 2 * canary) * 3,), 7, dtype=torch.int32, device=DEV)
    num = torch.full((4 + 2 * canary,), 7, dtype=torch.int32, device=DEV)
    out_mesh = (store[canary * 3:(canary + mt) * 3].view(mt, 3), num[canary:canary + 4])
    mesh, cut = _check(dims, D, Wt, C, max_triangles=mt, max_points=mp, out_mesh=out_mesh)
    lost = (full["tri"][:total] >= mp).any(axis=1)
    assert cut["num"].tolist() == [total, total, int(lost.sum()), 0] and 0 < lost.sum() < total
    assert (cut["tri"][:total][lost] == -1).all() and np.array_equal(cut["tri"][:total][~lost], full["tri"][:total][~lost])
    assert (store[:canary * 3] == 7).all() and (store[(canary + mt) * 3:] == 7).all()
    assert (num[:canary] == 7).all() and (num[canary + 4:] == 7).all()
    with pytest.raises(ValueError):
        mesh.check()
    vertices, normals, colours, triangles = mesh.to_host()
    assert len(vertices) == len(normals) == len(colours) == mp and np.array_equal(triangles, full["tri"][:total][~lost])


def test_overrides_of_min_weight_and_max_points():
    """``extract_mesh(min_weight=, max_points=)`` is the mesh of a volume with those parameters; the volume's own stay."""
    dims = (21, 13, 6)
    D, _, C = _random(dims, 31)
    Wt = np.random.RandomState(32).randint(0, 4, size=21 * 13 * 6)
    vol, want = _volumes(dims, D, Wt, C)
    want.p.update(min_weight=2, max_points=300)
    expected = mref.mesh(want, 5000)
    _same(vol.extract_mesh(min_weight=2, max_points=300, max_triangles=5000), expected)
    assert vol.params.min_weight == 1 and expected["num"][2] > 0
    with pytest.raises(ValueError):
        vol.extract_mesh(max_triangles=(1 << 22) + 1)


def test_side_stream():
    stream = torch.cuda.Stream(device=DEV)
    dims = (63, 5, 3)
    D, Wt, C = _random(dims, 61)
    torch.cuda.synchronize()
    _, out = _check(dims, D, Wt, C, stream=stream)
    assert out["num"][0] > 0


def test_mesh_replays_from_a_graph():
    """One chain of kernels and two prefix sums: the replay follows the volume as it then stands."""
    dims = (17, 16, 5)
    D, Wt, C = _random(dims, 71)
    vol, want = _volumes(dims, D, Wt, C)
    side = torch.cuda.Stream(device=DEV)
    with torch.cuda.stream(side):                             # (warm up outside the capture: the scratch plane is allocated here)
        vol.extract_mesh(max_triangles=8192)
    side.synchronize()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        mesh = vol.extract_mesh(max_triangles=8192)
    for seed in (71, 72):
        D, Wt, _ = _random(dims, seed)
        want.D, want.W = D, Wt
        vol.D.copy_(_dev(D))
        vol.W.copy_(_dev(Wt))
        graph.replay()
        torch.cuda.synchronize()
        _same(mesh, mref.mesh(want, 8192))


def test_save_ply_round_trips(tmp_path):
    dims = (9, 8, 7)
    D, Wt, C = _random(dims, 81)
    mesh, out = _check(dims, D, Wt, C)
    k, kt = mesh.check()
    assert (k, kt) == (int(out["surface"]["num"][0]), int(out["num"][0]))
    path = tmp_path / "mesh.ply"
    mesh.save_ply(str(path))
    raw = path.read_bytes()
    end = raw.index(b"end_header\n") + len(b"end_header\n")
    header = raw[:end].decode("ascii").split("\n")
    assert header[:2] == ["ply", "format binary_little_endian 1.0"]
    assert header[2] == "element vertex %d" % k and "element face %d" % kt in header
    assert [line for line in header if line.startswith("property")] == [
        "property float x", "property float y", "property float z", "property float nx", "property float ny", "property float nz",
        "property uchar red", "property uchar green", "property uchar blue", "property list uchar int vertex_indices"]
    vertex = np.frombuffer(raw, dtype=[("xyz", "<f4", (3,)), ("n", "<f4", (3,)), ("rgb", "u1", (3,))], count=k, offset=end)
    face = np.frombuffer(raw, dtype=[("n", "u1"), ("v", "<i4", (3,))], count=kt, offset=end + k * 27)
    assert len(raw) == end + k * 27 + kt * 13
    assert vertex["xyz"].tobytes() == out["surface"]["xyz"][:k].tobytes()
    assert vertex["n"].tobytes() == out["surface"]["normal"][:k].tobytes()
    assert np.array_equal(vertex["rgb"], np.rint(out["surface"]["rgb"][:k].astype(np.float64) * 255).astype(np.uint8))
    assert (face["n"] == 3).all() and np.array_equal(face["v"], out["tri"][:kt])


def test_every_error_code():
    from regnet_for_3d_grasping_amd import _lib
    L = _lib.lib
    SHAPE, NULL, UNSUPPORTED = -1, -2, -3
    buf = torch.zeros((4096,), dtype=torch.float32, device=DEV)
    p = buf.data_ptr()
    before = buf.clone()
    assert L.regnet_tsdf_mesh_blocks(3, 3, 29) == 2 and L.regnet_tsdf_mesh_blocks(3, 0, 29) == -1
    assert L.regnet_tsdf_mesh_blocks(1 << 14, 1 << 14, 2) == -1 and L.regnet_tsdf_mesh_scratch_bytes(1 << 14, 1 << 14, 1) == 4 << 28
    assert L.regnet_tsdf_mesh_scratch_bytes(2, 3, 4) == 96 and L.regnet_tsdf_mesh_scratch_bytes(2, 3, -4) == -1
    edges = (ctypes.c_int8 * 16)()
    assert L.regnet_tsdf_mesh_case(256, edges) == SHAPE and L.regnet_tsdf_mesh_case(-1, edges) == SHAPE
    assert L.regnet_tsdf_mesh_case(1, None) == NULL and L.regnet_tsdf_mesh_case(1, edges) == 0 and list(edges)[:4] == [0, 1, 2, -1]

    def count(volume=p, dims=(2, 2, 2), min_weight=1, tri_block_counts=p, num_tri=p):
        return L.regnet_tsdf_mesh_count(volume, *dims, min_weight, tri_block_counts, num_tri, None)
    assert count(dims=(2, 2, -1)) == SHAPE and count(min_weight=0) == SHAPE and count(dims=(1 << 28, 2, 1)) == UNSUPPORTED
    for name in ("volume", "tri_block_counts", "num_tri"):
        assert count(**{name: None}) == NULL, name

    def emit(volume=p, dims=(2, 2, 2), min_weight=1, block_counts=p, block_base=p, K_source=p, tri_block_counts=p, tri_block_base=p,
             max_triangles=8, scratch=p, tri=p, num_tri=p):
        return L.regnet_tsdf_mesh_emit(volume, *dims, min_weight, block_counts, block_base, K_source, tri_block_counts,
                                       tri_block_base, max_triangles, scratch, tri, num_tri, None)
    assert emit(dims=(0, 2, 2)) == SHAPE and emit(min_weight=0) == SHAPE and emit(max_triangles=0) == SHAPE
    assert emit(max_triangles=(1 << 22) + 1) == UNSUPPORTED and emit(dims=(1 << 28, 2, 1)) == UNSUPPORTED
    for name in ("volume", "block_counts", "block_base", "K_source", "tri_block_counts", "tri_block_base", "scratch", "tri", "num_tri"):
        assert emit(**{name: None}) == NULL, name
    torch.cuda.synchronize()
    assert torch.equal(buf, before)                           # every error was returned before any launch
