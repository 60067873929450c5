"""``GraspDetector(volume=..., mesh=True)`` and ``(track=..., mesh=True)`` end to end on the two 160 x 120 views of
tests/test_gpu_detect_fused.py and the three frames of tests/test_gpu_detect_track.py: the record's mesh keys are
``Volume.extract_mesh`` of the same views, every other key is the run without the option, the CLI flags and the PLY beside the
record, and the tracked volume's mesh is closed away from the border of observed space."""
import collections
import contextlib
import io

import numpy as np
import pytest

from . import tsdf_mesh_reference as mref
from . import tsdf_reference as ref
from .test_gpu_detect_fused import SEED, _run, _same_state, parts  # noqa: F401  (the module-scoped fixture)
from .test_gpu_detect_track import TRACK, sequence
from .test_gpu_detect_tsdf import VOLUME, _equal

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def test_the_records_mesh_is_extract_mesh_of_the_same_views(parts):  # noqa: F811
    from regnet_for_3d_grasping_amd import detect, tsdf
    mv = parts[2]
    got, got_state = _run(parts, mv, volume=VOLUME, mesh=True)
    plain, plain_state = _run(parts, mv, volume=VOLUME)
    assert tuple(plain) == detect.RESULT_KEYS + detect.TSDF_KEYS
    assert tuple(got) == detect.RESULT_KEYS + detect.TSDF_KEYS + detect.TSDF_MESH_KEYS
    _equal(got, plain, tuple(plain))                          # every other key is the run without the option
    assert _same_state(got_state, plain_state)
    surface, mesh = tsdf.fuse_volume(mv, None, VOLUME, device=DEV, mesh=True)
    assert mesh.surface is surface and surface.volume is not None
    k, kt = mesh.check()
    vertices, normals, colours, triangles = mesh.to_host()
    assert got["tsdf_triangles"].dtype == np.int32 and got["tsdf_triangles"].shape == (kt, 3) and kt > 2000
    for key, want in zip(detect.TSDF_MESH_KEYS, (triangles, vertices, normals, colours)):
        assert got[key].dtype == want.dtype and got[key].tobytes() == want.tobytes(), key
    assert got["tsdf_vertices"].shape == (k, 3) == got["tsdf_vertex_normals"].shape == got["tsdf_vertex_colors"].shape
    assert k == int(got["tsdf_num"][0]) and got["tsdf_triangles"].min() >= 0 and got["tsdf_triangles"].max() < k
    # the same through the dict form of the option
    again, _ = _run(parts, mv, volume=dict(VOLUME, mesh=True))
    _equal(again, got, tuple(got))


def test_the_cli_flags_and_the_ply_beside_the_record(parts, tmp_path):  # noqa: F811
    from regnet_for_3d_grasping_amd import detect, fusion
    parser = detect.build_parser()
    required = ["--folder", "x", "--load-score-path", "a", "--load-region-path", "b"]
    args = parser.parse_args(required)
    assert args.tsdf_mesh is False and args.tsdf_mesh_ply is False
    assert parser.parse_args(required + ["--tsdf", "--tsdf-mesh"]).tsdf_mesh is True
    args = parser.parse_args(required + ["--tsdf", "--tsdf-mesh-ply"])
    with pytest.raises(ValueError, match="mesh"):
        detect.GraspDetector(parts[0], parts[1], mesh=True)
    assert detect.GraspDetector(parts[0], parts[1], volume=detect.volume_from_args(args)).mesh is False
    detector = detect.GraspDetector(parts[0], parts[1], volume=VOLUME, mesh=args.tsdf_mesh, mesh_ply=args.tsdf_mesh_ply)
    assert detector.mesh and detector.mesh_ply
    folder = tmp_path / "real_data"
    folder.mkdir()
    path = str(folder / "cell.npz")
    fusion.save_npz(path, parts[2])
    np.random.seed(SEED)
    with contextlib.redirect_stdout(io.StringIO()):
        out, saved = detector.detect_file(path)
    assert saved == str(tmp_path / "real_data_predict" / "cell.p")
    raw = (tmp_path / "real_data_predict" / "cell.ply").read_bytes()
    k, kt = len(out["tsdf_vertices"]), len(out["tsdf_triangles"])
    end = raw.index(b"end_header\n") + len(b"end_header\n")
    assert b"element vertex %d\n" % k in raw[:end] and b"element face %d\n" % kt in raw[:end]
    assert len(raw) == end + 27 * k + 13 * kt
    face = np.frombuffer(raw, dtype=[("n", "u1"), ("v", "<i4", (3,))], count=kt, offset=end + 27 * k)
    assert np.array_equal(face["v"], out["tsdf_triangles"])


def test_the_tracked_volumes_mesh_is_closed_in_its_interior(parts):  # noqa: F811
    """After the third frame: an edge of the mesh is used by two triangles, once in each direction, unless it lies on the border
    of observed space -- one of its two vertices sits on a voxel edge that touches a cell with a corner that is not usable, or
    the volume's faces."""
    from regnet_for_3d_grasping_amd import detect
    frames, _ = sequence()
    detector = detect.GraspDetector(parts[0], parts[1], track=dict(TRACK, mesh=True), volume=VOLUME)
    assert detector.mesh
    for frame in frames:
        np.random.seed(SEED)
        record = detector.detect(frame)
    assert tuple(record) == detect.RESULT_KEYS + detect.TSDF_KEYS + detect.TRACK_KEYS + detect.TSDF_MESH_KEYS
    assert int(record["track_status"]) == 1
    tri = record["tsdf_triangles"]
    assert len(tri) > 2000
    use = collections.Counter()
    for a, b, c in tri.tolist():
        for x, y in ((a, b), (b, c), (c, a)):
            use[(x, y)] += 1
    assert all(n == 1 for n in use.values())                  # oriented: no directed edge twice
    # the cells that are meshed and the key of every vertex row, from the volume itself through the numpy restatement
    vol = detector.tsdf_volume
    nx, ny, nz = vol.params.dims
    want = ref.Volume(**VOLUME)
    want.D, want.W = vol.D.cpu().numpy(), vol.W.cpu().numpy()
    keys = want.extract()["keys"]
    assert len(keys) == len(record["tsdf_vertices"])
    ok = mref.usable(want).reshape(nz, ny, nx)
    meshed = np.ones((nz - 1, ny - 1, nx - 1), dtype=bool)
    for dz in (0, 1):
        for dy in (0, 1):
            for dx in (0, 1):
                meshed &= ok[dz:nz - 1 + dz, dy:ny - 1 + dy, dx:nx - 1 + dx]
    # a vertex is interior when the four cells round its voxel edge all exist and are meshed
    interior = np.ones(len(keys), dtype=bool)
    for v, key in enumerate(keys.tolist()):
        l, axis = divmod(key, 3)
        base = [l % nx, l // nx % ny, l // (nx * ny)]
        others = [k for k in range(3) if k != axis]
        for da in (-1, 0):
            for db in (-1, 0):
                cell = list(base)
                cell[others[0]] += da
                cell[others[1]] += db
                inside = min(cell) >= 0 and cell[0] < nx - 1 and cell[1] < ny - 1 and cell[2] < nz - 1
                if not inside or not meshed[cell[2], cell[1], cell[0]]:
                    interior[v] = False
    assert interior.sum() > 1000
    open_interior = [(x, y) for (x, y) in use if (y, x) not in use and interior[x] and interior[y]]
    assert not open_interior, open_interior[:5]
