"""What simplifying the TSDF mesh costs on the MI355X (tsdf.Mesh.simplify, csrc/mesh_simplify.hip) -> profiles/mesh_simplify.txt.

Two steps, each a fresh child process under its own time limit; the driver stops at the first one that fails:
  kernels  the two rendered 640 x 480 views and the 320^3 volume of scripts/bench_tsdf.py, meshed by ``extract_mesh``; for the
           factors 3, 4 and 8 ``simplify`` alone (two fills and eight launches, timed as one call: the entry point is one call and
           is not broken down per launch here), the triangle and vertex counts before and after, the bytes the call must move
           at least (a count) as the bound it is held against, and the host route beside it: the download of the mesh and
           ``np.unique`` on the keys, on a host clock.
  detect   one GraspDetector.detect of the two-view MultiView with ``volume`` and ``mesh`` with and without ``mesh_cell``,
           alternated, on a host clock.
Warm-up first, then the median of repeated runs with their min / max.

    python scripts/bench_mesh_simplify.py [--out profiles/mesh_simplify.txt]
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
FACTORS = (3, 4, 8)


def host_simplify(xyz, tri, origin, cell, grid):
    """The host route on downloaded arrays: cells in float32, ``np.unique`` on the vertices' cells and on the triangles' keys
    -> (vertices, triangles) kept.  Positions, normals and colours are not averaged: it does less than the device."""
    import numpy as np
    a = (xyz - origin) / np.float32(cell)
    i = np.floor(a).astype(np.int64)
    c = (i[:, 2] * grid[1] + i[:, 1]) * grid[0] + i[:, 0]
    t = c[tri]
    keep = (t[:, 0] != t[:, 1]) & (t[:, 1] != t[:, 2]) & (t[:, 2] != t[:, 0])
    t = t[keep]
    lo = np.argmin(t, axis=1)
    rows = np.arange(len(t))
    key = (t[rows, lo] << 42) | (t[rows, (lo + 1) % 3] << 21) | t[rows, (lo + 2) % 3]
    kept = np.unique(key)
    used = np.unique(np.stack([kept >> 42, (kept >> 21) & 0x1fffff, kept & 0x1fffff]))
    return len(used), len(kept)


def step_kernels(lines):
    import numpy as np
    import torch
    from regnet_for_3d_grasping_amd import _lib, tsdf
    mv, views = scene()
    params = tsdf.TsdfParams(origin=ORIGIN)
    vol = tsdf.Volume(params, DEV)
    for v in (0, 1):
        vol.integrate(views[v], mv.poses[v])
    mesh = vol.extract_mesh()
    k, kt = mesh.check()
    med = statistics.median
    lines.append("volume %d x %d x %d voxels of %g m, two views integrated: %d vertices, %d triangles (rows %d, max_triangles %d)"
                 % (params.dims + (params.voxel, k, kt, params.max_points, mesh.max_triangles)))
    same = True
    for factor in FACTORS:
        simple = mesh.simplify(factor=factor)
        kv, kts = simple.check()
        report = simple.report.cpu().numpy()
        cells = simple.grid[0] * simple.grid[1] * simple.grid[2]
        t_call = sorted(timed(lambda: mesh.simplify(factor=factor), 3, 20))
        workspace = int(_lib.lib.regnet_mesh_simplify_workspace_bytes(cells, mesh.max_triangles))
        slots = int(_lib.lib.regnet_mesh_simplify_table_slots(mesh.max_triangles))
        # a COUNT of the bytes the call cannot avoid: the two fills (84 B per cell, 12 B per slot, 4 B per cell), the 36 B of
        # every source vertex and the 12 B of every source triangle once, and the outputs' rows (40 B and 12 B) to their capacity
        mv_rows, mt_rows = simple.sizes()
        least = 88 * cells + 12 * slots + 36 * k + 12 * kt + 40 * mv_rows + 12 * mt_rows
        bound_ms = least / PEAK_BYTES_PER_S * 1e3
        lines.append("  factor %d: cell %g m, grid %d x %d x %d = %d cells, workspace %.1f MB" % (
            (factor, simple.cell) + simple.grid + (cells, workspace / 1e6)))
        lines.append("    simplify          %s  (two fills + eight launches, one call; not broken down per launch)" % fmt(t_call))
        lines.append("    byte bound        %.4f ms for %.1f MB at 8 TB/s (a count: fills %.1f MB, source %.1f MB, output rows %.1f MB): "
                     "the call is %.1f x that -- its launches are short and serial, so where the rest goes is only supposed "
                     "(launch gaps and the atomics of contended cells), no counter run was made" % (
                         bound_ms, least / 1e6, (88 * cells + 12 * slots) / 1e6, (36 * k + 12 * kt) / 1e6,
                         (40 * mv_rows + 12 * mt_rows) / 1e6, med(t_call) / bound_ms))
        lines.append("    result            %d -> %d triangles (%.1f x fewer), %d -> %d vertices; collapsed %d, duplicate %d, "
                     "occupied cells %d" % (kt, kts, kt / max(kts, 1), k, kv, report[9], report[10], report[3]))
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        xyz, tri = mesh.surface.xyz[:k].cpu().numpy(), mesh.triangles[:kt].cpu().numpy()
        t1 = time.perf_counter()
        hv, ht = host_simplify(xyz, tri, vol.origin, simple.cell, simple.grid)
        t2 = time.perf_counter()
        ok = (hv, ht) == (kv, kts)
        same = same and ok
        lines.append("    host route        download of vertices and triangles %.1f ms, cells + np.unique on the keys %.1f ms, one "
                     "run, host clock (no averaging of positions, normals, colours): %.0f x simplify;  its %d vertices and %d "
                     "triangles %s the device's" % ((t1 - t0) * 1e3, (t2 - t1) * 1e3, (t2 - t0) * 1e3 / med(t_call), hv, ht,
                                                    "equal" if ok else "DIFFER FROM"))
    return same


def step_detect(lines):
    import contextlib
    import io

    import numpy as np
    import torch
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
    meshed = detect.GraspDetector(score_net, region_net, volume={"origin": ORIGIN}, mesh=True)
    simple = detect.GraspDetector(score_net, region_net, volume={"origin": ORIGIN}, mesh_cell=4 * 0.002)

    def once(detector):
        np.random.seed(1234)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = detector.detect(mv)
        return (time.perf_counter() - t0) * 1e3, out
    for _ in range(3):
        once(meshed)
        once(simple)
    times = {"mesh": [], "cell": []}
    for _ in range(15):
        ms, full = once(meshed)
        times["mesh"].append(ms)
        ms, out = once(simple)
        times["cell"].append(ms)
    a, b = sorted(times["mesh"]), sorted(times["cell"])
    diff = statistics.median(b) - statistics.median(a)
    lines.append("GraspDetector.detect of two 640 x 480 views with volume and mesh, host clock:  full mesh (%d triangles, %d vertices "
                 "into the record) %s;  with mesh_cell = 4 voxels (%d triangles, %d vertices) %s;  difference of the medians %+.3f "
                 "ms = %+.2f%%" % (len(full["tsdf_triangles"]), len(full["tsdf_vertices"]), fmt(a), len(out["tsdf_triangles"]),
                                   len(out["tsdf_vertices"]), fmt(b), diff, 100.0 * diff / statistics.median(a)))
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
    parser.add_argument("--out", default=os.path.join(REPO, "profiles", "mesh_simplify.txt"))
    parser.add_argument("--step", choices=[name for name, _ in STEPS], help="(internal) run one step in this process")
    parser.add_argument("--step-out", help="(internal) where the step leaves its lines")
    args = parser.parse_args()
    if args.step:
        sys.exit(run_step(args.step, args.step_out))
    import torch
    lines = ["Mesh simplification on the device (scripts/bench_mesh_simplify.py): %s, torch %s; two rendered 640 x 480 views at 320^3; "
             "median of HIP-event times unless a host clock is named" % (
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
