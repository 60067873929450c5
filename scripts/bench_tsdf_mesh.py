"""What the TSDF volume's triangle mesh costs on the MI355X (tsdf.Volume.extract_mesh, csrc/tsdf_mesh.hip) -> profiles/tsdf_mesh.txt.

Two steps, each a fresh child process under its own time limit; the driver stops at the first one that fails:
  kernels  the two rendered 640 x 480 views and the 320^3 volume of scripts/bench_tsdf.py: ``extract_mesh`` whole beside
           ``extract`` of the same state, alternated; its passes apart (count, ``torch.cumsum``, and the emit call: row lookup,
           cells, tail); the triangle count; one pass over D and W (8 B per voxel at 8 TB/s) as the bound it is held against;
           and the host route: the download of D and W and a vectorised numpy marching cubes with the table of
           tests/tsdf_mesh_reference.py (``skimage.measure.marching_cubes`` instead when that package is importable), whose
           triangles are compared with the device's.  HIP-event times; the host route on a host clock.
  detect   one GraspDetector.detect of the two-view MultiView with ``volume`` with and without ``mesh``, alternated.
Warm-up first, then the median of repeated runs with their min / max.

    python scripts/bench_tsdf_mesh.py [--out profiles/tsdf_mesh.txt]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_outliers import fmt, timed  # noqa: E402
from bench_tsdf import DEV, ORIGIN, PEAK_BYTES_PER_S, scene  # noqa: E402

STEPS = (("kernels", 420), ("detect", 420))     # (name, time limit in seconds)


def host_mesh(D, Wt, dims, min_weight):
    """Vectorised numpy marching cubes over the downloaded planes, by the contract's rules -> (T,3) int64 of rows."""
    import numpy as np
    from tests import tsdf_mesh_reference as mref
    nx, ny, nz = dims
    D, Wt = D.reshape(nz, ny, nx), Wt.reshape(nz, ny, nx)
    ok = (Wt >= min_weight) & (D < 1)
    neg = D < 0
    meshed = np.ones((nz - 1, ny - 1, nx - 1), dtype=bool)
    case = np.zeros((nz - 1, ny - 1, nx - 1), dtype=np.int32)
    for c, (dx, dy, dz) in enumerate(mref.CORNERS):
        sl = (slice(dz, nz - 1 + dz), slice(dy, ny - 1 + dy), slice(dx, nx - 1 + dx))
        meshed &= ok[sl]
        case |= neg[sl].astype(np.int32) << c
    case[~meshed] = 0
    iz, iy, ix = np.nonzero(mref.TRIANGLES[case] > 0)
    cs = case[iz, iy, ix]
    cell = (iz.astype(np.int64) * ny + iy) * nx + ix
    # the kept candidates' keys, ascending: a row is a key's rank
    keys = []
    for a, step in enumerate((1, nx, nx * ny)):
        lo = [slice(None)] * 3
        hi = [slice(None)] * 3
        lo[2 - a], hi[2 - a] = slice(0, -1), slice(1, None)
        kept = ok[tuple(lo)] & ok[tuple(hi)] & (neg[tuple(lo)] != neg[tuple(hi)])
        z, y, x = np.nonzero(kept)
        keys.append(3 * ((z.astype(np.int64) * ny + y) * nx + x) + a)
    keys = np.sort(np.concatenate(keys))
    corner = np.array([dx + dy * nx + dz * nx * ny for dx, dy, dz in mref.CORNERS], dtype=np.int64)
    edge_c, edge_a = np.array([e[0] for e in mref.EDGES]), np.array([e[1] for e in mref.EDGES])
    out = []
    for t in range(mref.MAX_TRIANGLES_PER_CASE):
        has = mref.TRIANGLES[cs] > t
        e = mref.TABLE[cs[has], 3 * t:3 * t + 3].astype(np.int64)
        key = 3 * (cell[has, None] + corner[edge_c[e]]) + edge_a[e]
        out.append((cell[has], np.full(has.sum(), t), np.searchsorted(keys, key)))
    cells, ts, rows = (np.concatenate([o[j] for o in out]) for j in range(3))
    order = np.lexsort((ts, cells))
    return rows[order], len(keys)


def step_kernels(lines):
    import numpy as np
    import torch
    from regnet_for_3d_grasping_amd import _lib, tsdf
    mv, views = scene()
    params = tsdf.TsdfParams(origin=ORIGIN)
    vol = tsdf.Volume(params, DEV)
    n = vol.D.numel()
    nx, ny, nz = params.dims
    for v in (0, 1):
        vol.integrate(views[v], mv.poses[v])
    med = statistics.median
    mesh = vol.extract_mesh()
    k, kt = mesh.check()
    mt = mesh.max_triangles
    s = mesh.surface
    out = (s.xyz, s.rgb, s.normal, s.weight, s.num)
    out_mesh = (mesh.triangles, mesh.num_triangles)
    lines.append("volume %d x %d x %d voxels of %g m, two views integrated: %d surface rows, %d triangles (max_triangles %d); "
                 "scratch plane %.0f MB" % (params.dims + (params.voxel, k, kt, mt, 4 * n / 1e6)))
    t_plain, t_mesh = [], []
    for _ in range(5):                               # alternated: both see the same neighbours on the machine
        t_plain += timed(lambda: vol.extract(out=out), 2, 8)
        t_mesh += timed(lambda: vol.extract_mesh(out=out, out_mesh=out_mesh), 2, 8)
    t_plain, t_mesh = sorted(t_plain), sorted(t_mesh)
    read_ms = 8 * n / PEAK_BYTES_PER_S * 1e3
    lines.append("    extract           %s" % fmt(t_plain))
    lines.append("    extract_mesh      %s = %.2f x extract;  one pass over D and W (%.0f MB) at 8 TB/s: %.3f ms, the mesh's "
                 "share of the call (extract_mesh - extract) is %.1f x that" % (
                     fmt(t_mesh), med(t_mesh) / med(t_plain), 8 * n / 1e6, read_ms, (med(t_mesh) - med(t_plain)) / read_ms))
    # the passes apart, on the arrays of one extraction
    block_counts = torch.empty((int(_lib.lib.regnet_tsdf_blocks(nx, ny, nz)),), dtype=torch.int32, device=DEV)
    _lib.call("regnet_tsdf_count", vol.data, vol.data.data_ptr(), nx, ny, nz, params.min_weight, block_counts.data_ptr(),
              s.num.data_ptr())
    base = torch.cumsum(block_counts, 0, dtype=torch.int32) - block_counts
    _lib.call("regnet_tsdf_emit_f32", vol.data, vol.data.data_ptr(), nx, ny, nz, vol.origin.ctypes.data, params.voxel,
              params.min_weight, block_counts.data_ptr(), base.data_ptr(), params.max_points, *(t.data_ptr() for t in out))
    tri_counts = torch.empty((int(_lib.lib.regnet_tsdf_mesh_blocks(nx, ny, nz)),), dtype=torch.int32, device=DEV)

    def count():
        _lib.call("regnet_tsdf_mesh_count", vol.data, vol.data.data_ptr(), nx, ny, nz, params.min_weight, tri_counts.data_ptr(),
                  mesh.num_triangles.data_ptr())
    count()
    tri_base = torch.cumsum(tri_counts, 0, dtype=torch.int32) - tri_counts

    def emit():
        _lib.call("regnet_tsdf_mesh_emit", vol.data, vol.data.data_ptr(), nx, ny, nz, params.min_weight, block_counts.data_ptr(),
                  base.data_ptr(), s.num.data_ptr(), tri_counts.data_ptr(), tri_base.data_ptr(), mt, vol.mesh_scratch.data_ptr(),
                  mesh.triangles.data_ptr(), mesh.num_triangles.data_ptr())
    t_count, t_emit = timed(count, 3, 20), timed(emit, 3, 20)
    t_sum = timed(lambda: torch.cumsum(tri_counts, 0, dtype=torch.int32) - tri_counts, 3, 20)
    lines.append("    mesh count pass   %s = %.1f x the byte bound  (clear + count: the eight corners of every cell)" % (
        fmt(t_count), med(t_count) / read_ms))
    lines.append("    torch.cumsum      %s  (%d blocks of 256 cells)" % (fmt(t_sum), tri_counts.numel()))
    lines.append("    mesh emit call    %s  (row lookup, cells and tail: three launches, not broken down; blocks without a "
                 "candidate or a triangle leave at once, %d of %d blocks have triangles; the tail writes %d rows of -1)" % (
                     fmt(t_emit), int((tri_counts > 0).sum()), tri_counts.numel(), mt - kt))
    emit()
    assert mesh.check() == (k, kt)
    # the host route
    device_tri = mesh.triangles[:kt].cpu().numpy()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    D, Wt = vol.D.cpu().numpy(), vol.W.cpu().numpy()
    t1 = time.perf_counter()
    try:
        from skimage import measure
        verts, faces, _, _ = measure.marching_cubes(np.where(Wt >= params.min_weight, D, 1.0).reshape(nz, ny, nx), 0.0)
        t2 = time.perf_counter()
        lines.append("host route: download of D and W %.1f ms, skimage.measure.marching_cubes %.1f ms (%d triangles; its own "
                     "masking and table: not compared)" % ((t1 - t0) * 1e3, (t2 - t1) * 1e3, len(faces)))
    except ImportError:
        host_tri, host_rows = host_mesh(D, Wt, params.dims, params.min_weight)
        t2 = time.perf_counter()
        same = host_rows == k and host_tri.shape == device_tri.shape and bool((host_tri == device_tri).all())
        lines.append("host route (no skimage on this machine): download of D and W %.1f ms, vectorised numpy marching cubes with "
                     "the restatement's table %.1f ms, one run, host clock: %.0f x extract_mesh;  its %d triangles %s the device's" % (
                         (t1 - t0) * 1e3, (t2 - t1) * 1e3, (t2 - t0) * 1e3 / med(t_mesh), len(host_tri),
                         "equal" if same else "DIFFER FROM"))
        return same
    return True


def step_detect(lines):
    import numpy as np
    import torch
    import contextlib
    import io
    from regnet_for_3d_grasping_amd import detect, pipeline, synthetic
    from regnet_for_3d_grasping_amd.get_regiondataset import get_grasp_allobj
    mv, _ = scene()
    score_net, region_net = pipeline.build_models(DEV)
    score_net.eval()
    region_net.eval()
    np.random.seed(1234)                             # the heads of the seeded networks calibrated as scripts/bench_tsdf.py does
    pc = detect.GraspDetector(score_net, region_net).ingest(mv).pc
    synthetic.calibrate_score_head(score_net, pc)
    with torch.no_grad():
        feat, score, _ = score_net(pc)
    np.random.seed(41)
    g = get_grasp_allobj(pc, score, detect.TEST_PARAMS, [], True)

    def region():
        with contextlib.redirect_stdout(io.StringIO()), torch.no_grad():
            return region_net(g[3], g[5], g[2], g[4], g[0], g[1], pc, feat, detect.GRIPPER_PARAMS, None, [])
    np.random.seed(5)
    synthetic.calibrate_region_head(region_net, region)
    plain = detect.GraspDetector(score_net, region_net, volume={"origin": ORIGIN})
    meshed = detect.GraspDetector(score_net, region_net, volume={"origin": ORIGIN}, mesh=True)

    def once(detector):
        np.random.seed(1234)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = detector.detect(mv)
        return (time.perf_counter() - t0) * 1e3, out
    for _ in range(3):
        once(plain)
        once(meshed)
    times = {"plain": [], "mesh": []}
    for _ in range(15):
        times["plain"].append(once(plain)[0])
        ms, out = once(meshed)
        times["mesh"].append(ms)
    a, b = sorted(times["plain"]), sorted(times["mesh"])
    diff = statistics.median(b) - statistics.median(a)
    lines.append("GraspDetector.detect of two 640 x 480 views with volume, host clock:  without mesh %s;  with mesh (%d triangles and %d vertices downloaded into the record) %s;  difference "
                 "of the medians %+.3f ms = %+.2f%%" % (fmt(a), len(out["tsdf_triangles"]), len(out["tsdf_vertices"]), fmt(b), diff,
                                                        100.0 * diff / statistics.median(a)))
    return True


def run_step(name, path):
    import torch
    assert torch.cuda.is_available(), "this measurement needs the MI355X"
    lines = []
    ok = {"kernels": step_kernels, "detect": step_detect}[name](lines)
    with open(path, "w") as f:
        json.dump(lines, f)
    return 0 if ok else 1


def main():
    parser = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    parser.add_argument("--out", default=os.path.join(REPO, "profiles", "tsdf_mesh.txt"))
    parser.add_argument("--step", choices=[name for name, _ in STEPS], help="(internal) run one step in this process")
    parser.add_argument("--step-out", help="(internal) where the step leaves its lines")
    args = parser.parse_args()
    if args.step:
        sys.exit(run_step(args.step, args.step_out))
    import torch
    lines = ["TSDF triangle mesh on the device (scripts/bench_tsdf_mesh.py): %s, torch %s; two rendered 640 x 480 views; median of "
             "HIP-event times unless a host clock is named" % (
                 torch.cuda.get_device_name(0) if torch.cuda.is_available() else "no GPU", torch.__version__), ""]
    status = 0
    for name, limit in STEPS:
        part = args.out + "." + name + ".json"
        try:
            status = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", name, "--step-out", part],
                                    timeout=limit).returncode
        except subprocess.TimeoutExpired:
            status = 124
        if os.path.exists(part):
            with open(part) as f:
                lines += json.load(f)
            os.remove(part)
        if status != 0:                              # nothing more is started on the GPU after a step that failed
            lines.append("step %s ended with status %d: stopped here" % (name, status))
            break
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines).rstrip() + "\n")
    print("\n".join(lines))
    sys.exit(status)


if __name__ == "__main__":
    main()
