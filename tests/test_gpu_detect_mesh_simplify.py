"""``GraspDetector(volume=..., mesh_cell=...)`` end to end on the two 160 x 120 views of tests/test_gpu_detect_fused.py: the
record's mesh keys are then ``Mesh.simplify`` of the same views and ``tsdf_mesh_report`` is added, every other key is the run
without the option, and without ``mesh_cell`` the mesh keys are the full mesh's, byte for byte; the CLI flag and the PLY."""
import contextlib
import io

import numpy as np
import pytest

from .test_gpu_detect_fused import SEED, _run, _same_state, parts  # noqa: F401  (the module-scoped fixture)
from .test_gpu_detect_tsdf import VOLUME, _equal

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CELL = 4 * VOLUME["voxel"]


def test_the_records_mesh_is_the_simplified_mesh_of_the_same_views(parts):  # noqa: F811
    from regnet_for_3d_grasping_amd import detect, tsdf
    mv = parts[2]
    got, got_state = _run(parts, mv, volume=VOLUME, mesh_cell=CELL)
    full, full_state = _run(parts, mv, volume=VOLUME, mesh=True)
    assert tuple(full) == detect.RESULT_KEYS + detect.TSDF_KEYS + detect.TSDF_MESH_KEYS
    assert tuple(got) == tuple(full) + detect.TSDF_MESH_REPORT_KEYS == tuple(full) + ("tsdf_mesh_report",)
    _equal(got, full, detect.RESULT_KEYS + detect.TSDF_KEYS)  # the networks saw the full surface
    assert _same_state(got_state, full_state)
    # without mesh_cell the mesh keys are extract_mesh's, as they were
    surface, mesh = tsdf.fuse_volume(mv, None, VOLUME, device=DEV, mesh=True)
    assert type(mesh) is tsdf.Mesh
    vertices, normals, colours, triangles = mesh.to_host()
    for key, want in zip(detect.TSDF_MESH_KEYS, (triangles, vertices, normals, colours)):
        assert full[key].dtype == want.dtype and full[key].tobytes() == want.tobytes(), key
    # with it they are simplify's
    surface2, simple = tsdf.fuse_volume(mv, None, VOLUME, device=DEV, mesh=True, mesh_cell=CELL)
    assert isinstance(simple, tsdf.SimplifiedMesh) and simple.source.surface is surface2
    assert surface2.xyz.cpu().numpy().tobytes() == surface.xyz.cpu().numpy().tobytes()
    kv, kt = simple.check()
    vertices, normals, colours, triangles = simple.to_host()
    for key, want in zip(detect.TSDF_MESH_KEYS, (triangles, vertices, normals, colours)):
        assert got[key].dtype == want.dtype and got[key].tobytes() == want.tobytes(), key
    report = got["tsdf_mesh_report"]
    assert report.dtype == np.int32 and report.shape == (12,) and report.tobytes() == simple.report.cpu().numpy().tobytes()
    assert report[:3].tolist() == [kv, kv, 0] and report[5:9].tolist() == [kt, kt, 0, 0] and report[4] == 0
    assert report[6] + report[9] + report[10] + report[11] == len(full["tsdf_triangles"]) and report[11] == 0
    assert 0 < kt < len(full["tsdf_triangles"]) and 0 < kv < len(full["tsdf_vertices"]) and report[3] >= kv
    assert got["tsdf_triangles"].shape == (kt, 3) and got["tsdf_triangles"].min() == 0 and got["tsdf_triangles"].max() == kv - 1
    assert got["tsdf_vertices"].shape == got["tsdf_vertex_normals"].shape == got["tsdf_vertex_colors"].shape == (kv, 3)
    print("detect: %d -> %d triangles, %d -> %d vertices" % (len(full["tsdf_triangles"]), kt, len(full["tsdf_vertices"]), kv))
    # the same through the dict form of the option
    again, _ = _run(parts, mv, volume=dict(VOLUME, mesh_cell=CELL))
    _equal(again, got, tuple(got))


def test_the_cli_flag_and_the_ply_beside_the_record(parts, tmp_path):  # noqa: F811
    from regnet_for_3d_grasping_amd import detect, fusion
    parser = detect.build_parser()
    required = ["--folder", "x", "--load-score-path", "a", "--load-region-path", "b"]
    assert parser.parse_args(required).tsdf_mesh_cell is None
    args = parser.parse_args(required + ["--tsdf", "--tsdf-mesh-ply", "--tsdf-mesh-cell", repr(CELL)])
    assert args.tsdf_mesh_cell == CELL and args.tsdf_mesh is False
    with pytest.raises(ValueError, match="mesh"):
        detect.GraspDetector(parts[0], parts[1], mesh_cell=CELL)
    with pytest.raises(ValueError, match="mesh_cell"):
        detect.GraspDetector(parts[0], parts[1], volume=VOLUME, mesh_cell=0.0)
    detector = detect.GraspDetector(parts[0], parts[1], volume=VOLUME, mesh=args.tsdf_mesh, mesh_ply=args.tsdf_mesh_ply,
                                    mesh_cell=args.tsdf_mesh_cell)
    assert detector.mesh and detector.mesh_ply and detector.mesh_cell == CELL
    folder = tmp_path / "real_data"
    folder.mkdir()
    path = str(folder / "cell.npz")
    fusion.save_npz(path, parts[2])
    np.random.seed(SEED)
    with contextlib.redirect_stdout(io.StringIO()):
        out, saved = detector.detect_file(path)
    assert saved == str(tmp_path / "real_data_predict" / "cell.p") and "tsdf_mesh_report" in out
    raw = (tmp_path / "real_data_predict" / "cell.ply").read_bytes()
    k, kt = len(out["tsdf_vertices"]), len(out["tsdf_triangles"])
    assert (k, kt) == (int(out["tsdf_mesh_report"][0]), int(out["tsdf_mesh_report"][5]))
    end = raw.index(b"end_header\n") + len(b"end_header\n")
    assert b"element vertex %d\n" % k in raw[:end] and b"element face %d\n" % kt in raw[:end]
    assert len(raw) == end + 27 * k + 13 * kt
    face = np.frombuffer(raw, dtype=[("n", "u1"), ("v", "<i4", (3,))], count=kt, offset=end + 27 * k)
    assert np.array_equal(face["v"], out["tsdf_triangles"])
