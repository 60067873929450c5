"""The case table of the furthest-point-sampling tests (tests/fps_cases.py) against ``regnet_fps_plan``, the host function the
launcher, ``regnet_fps_workspace_bytes`` and ``regnet_fps_status_offset_bytes`` take everything from: every row reaches the
kernel it is there for, the table reaches every kernel the dispatch can reach, and around every threshold the workspace holds
what the selected kernel addresses.  No GPU: the plan sees 256 compute units where there is no device."""
import ctypes
import itertools
import os
import re

import pytest

from . import fps_cases as cases

OK, ERR_SHAPE, ERR_NULL, ERR_UNSUPPORTED = 0, -1, -2, -3
CUS = 256
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (points a workgroup holds at most, threads, points per thread): the instantiations of fps_resident_kernel; the sorting
# kernels take the same points per thread from their first size up
TILES = [(64, 64, 1), (128, 128, 1), (256, 256, 1), (512, 512, 1), (1024, 512, 2), (2048, 512, 4), (4096, 512, 8),
         (6144, 1024, 6), (8192, 1024, 8), (12288, 1024, 12), (16384, 1024, 16), (20480, 1024, 20), (25600, 1024, 25)]
COMPILED = ({("resident", t, p) for _, t, p in TILES} | {("cluster", 1024, p) for n, _, p in TILES if n > 4096} |
            {(f, 1024, p) for f in ("sorted", "coop") for n, _, p in TILES if n > 8192} | {("multi", 1024, 25), ("streaming", 1024, 0)})
# instantiations the dispatch compiles that no (B, N, M) reaches in the default build, with the reason
COMPILED_NOT_REACHED = {
    # cooperating workgroups start beyond 25 600 points and a scene is cut into G = ceil(N / 25600) >= 2 equal slices of
    # ceil(N / G) > 12 800 points: no slice fits 12 points per thread.  (Measurement builds that lower FPS_COOP_SLICE reach it.)
    ("coop", 1024, 12): "fps_cluster_kernel<12, 8, true>",
}

N_THRESHOLDS = [64, 128, 256, 512, 1024, 2048, 4096, 6144, 8192, 12288, 16384, 20480, 25600, 25601, 51200, 76800, 102400, 102401]
M_THRESHOLDS = [511, 512, 1023, 1024, 8192, 8193, 32767, 32768]
# 1, 8, and the first B at which G * B exceeds the compute units for G = 4, 3, 2, 1 (with the B below each)
B_VALUES = [1, 8, 64, 65, 85, 86, 128, 129, 256, 257]


def _sweep():
    ns = sorted({n + d for n in N_THRESHOLDS for d in (-1, 0, 1)})
    ms = sorted({1} | {m + d for m in M_THRESHOLDS for d in (-1, 0, 1)})
    return [(B, N, M) for B, N, M in itertools.product(B_VALUES, ns, ms) if M <= N]


@pytest.fixture(scope="module")
def swept():
    out = []
    for shape in _sweep():
        rc, plan = cases.query_plan(*shape)
        assert rc == OK, shape
        out.append((shape, plan))
    return out


def _key(plan):
    return plan["family"], plan["threads"], plan["ppt"]


ROWS = cases.all_rows()


@pytest.mark.parametrize("row", ROWS, ids=["%d-%d-%d" % r[:3] for r in ROWS])
def test_row_reaches_the_kernel_it_is_there_for(row):
    rc, plan = cases.query_plan(row.B, row.N, row.M)
    assert rc == OK
    assert (plan["family"], plan["ppt"]) == (row.family, row.ppt), plan
    # one row stays a matter of seconds, oracle included: no more distance evaluations than the streaming row's
    assert row.B * row.N * row.M <= 33500 * 33000


def test_workspace_holds_what_the_selected_kernel_addresses(swept):
    from regnet_for_3d_grasping_amd import _lib
    for (B, N, M), p in swept:
        where = ((B, N, M), p)
        G, ws, xchg, status = p["G"], p["workspace_bytes"], p["xchg_offset"], p["status_offset"]
        # the two queries of the binding are the plan's fields
        assert _lib.lib.regnet_fps_workspace_bytes(B, N, M) == ws, where
        assert _lib.lib.regnet_fps_status_offset_bytes(B, N, M) == status, where
        assert (status == -1) == (p["family"] != "coop"), where
        # the grid: G workgroups per scene, all of them resident at once when they wait for each other
        assert p["Bpad"] == (B if G == 1 else (B + 7) // 8 * 8) and p["grid"] == p["Bpad"] * G, where
        assert (G > 1) == (p["family"] in ("coop", "multi")) and 1 <= G <= 4 and (G == 1 or G * B <= CUS), where
        if p["family"] != "streaming":   # every point of a workgroup's slice has a register slot
            assert p["threads"] * p["ppt"] >= -(-N // G), where
        words = B * N * 4
        if p["family"] in ("resident", "sorted"):
            assert ws == 0 and xchg == -1, where
        elif p["family"] == "cluster":       # the sort's permutation
            assert ws >= words and xchg == -1, where
        elif p["family"] == "coop":          # permutation words, exchange area (zeroed with the status word), status word
            assert words <= xchg and xchg % 16 == 0, where
            assert xchg + B * cases.XCHG_BYTES <= status and status % 4 == 0 and status + 4 <= ws, where
            assert xchg + B * cases.XCHG_BYTES + cases.STATUS_BYTES <= ws, where
        elif p["family"] == "multi":         # 64 bytes of exchange slots per scene at the front
            assert xchg == 0 and B * 64 <= ws, where
        else:                                # the running distances
            assert p["family"] == "streaming" and ws >= words and xchg == -1, where


def test_table_reaches_every_kernel_the_dispatch_reaches(swept):
    reachable = {_key(p) for _, p in swept}
    covered = {_key(cases.query_plan(r.B, r.N, r.M)[1]) for r in ROWS}
    assert covered == reachable, "holes: %s" % sorted(reachable - covered)
    # ... and that is every instantiation the dispatch compiles but the ones listed with their reason
    assert reachable | set(COMPILED_NOT_REACHED) == COMPILED and not reachable & set(COMPILED_NOT_REACHED)
    # the per-wave kernel is reached only beyond the cluster kernel's LDS pick buffer; the multi-workgroup kernel by short runs
    assert all(M > 8192 and 8192 < N <= 25600 for (_, N, M), p in swept if p["family"] == "sorted")
    assert all(N > 25600 and (M < 1024 or M > 8192) for (_, N, M), p in swept if p["family"] == "multi")


def test_no_slice_of_cooperating_workgroups_fits_12_points_per_thread():
    for N in range(25601, 102401):
        rc, p = cases.query_plan(1, N, 1024)
        assert rc == OK and p["family"] == "coop" and p["ppt"] in (16, 20, 25) and -(-N // p["G"]) > 12288, (N, p)


def test_plan_returns_the_launchers_own_error_codes():
    from regnet_for_3d_grasping_amd import _lib
    zero = dict.fromkeys(cases.PLAN_FIELDS, 0)
    for shape, want in [((1, 10, 0), ERR_SHAPE), ((1, 10, 11), ERR_SHAPE), ((-1, 10, 5), ERR_SHAPE), ((1, 1 << 30, 5), ERR_UNSUPPORTED),
                        ((1, 1 << 30, 0), ERR_SHAPE), ((0, 1 << 30, 5), ERR_UNSUPPORTED)]:
        rc, plan = cases.query_plan(*shape)
        assert rc == want and dict(plan, family=0) == zero and plan["family"] is None, shape
        assert rc == _lib.lib.regnet_fps_f32(None, 0, 0, 0, *shape, None, None, None), shape
        assert _lib.lib.regnet_fps_workspace_bytes(*shape) == 0 and _lib.lib.regnet_fps_status_offset_bytes(*shape) == -1
    # an empty batch: success, nothing launched, no workspace
    rc, plan = cases.query_plan(0, 51200, 5120)
    assert rc == OK and plan == dict(zero, family=None, xchg_offset=-1, status_offset=-1)
    assert _lib.call("regnet_fps_plan", None, 1, 10, 5, None) == ERR_NULL
    assert cases.query_plan(1, (1 << 30) - 1, 5) == (OK, dict(family="streaming", threads=1024, ppt=0, G=1, Bpad=1, grid=1,
                                                               workspace_bytes=(1 << 32) + cases.XCHG_BYTES + 256,
                                                               xchg_offset=-1, status_offset=-1))


def test_plan_needs_no_device_pointer():
    """Host memory in, host memory out: the nine words are all the function touches."""
    from regnet_for_3d_grasping_amd import _lib
    buf = (ctypes.c_int64 * 11)(*([-5] * 11))
    assert _lib.call("regnet_fps_plan", None, 2, 51200, 5120, ctypes.addressof(buf) + 8) == OK
    assert buf[0] == -5 and buf[10] == -5 and list(buf[1:7]) == [4, 1024, 25, 2, 8, 16]


def test_pipeline_counts_the_plans_workgroups_per_scene():
    """``pipeline.sampling_workgroups_per_scene`` sizes the sampling launches from its own arithmetic.  It equals the plan's G
    for every scene up to 102 400 points.  Beyond, the two differ -- the plan takes ONE streaming workgroup, the pipeline counts
    ceil(N / 25600): a scheduling-only discrepancy (fewer scenes per launch than would fit) outside every measured shape,
    recorded here and in DESIGN.md and left as it is."""
    from regnet_for_3d_grasping_amd import pipeline
    for N in sorted(set(range(5120, 102401, 997)) | {n + d for n in N_THRESHOLDS[8:-1] for d in (-1, 0, 1) if n + d <= 102400}):
        for M in (512, 5120):
            assert pipeline.sampling_workgroups_per_scene(N) == cases.query_plan(1, N, M)[1]["G"], (N, M)
    for M in (512, 5120):
        assert cases.query_plan(1, 102401, M)[1]["G"] == 1 and pipeline.sampling_workgroups_per_scene(102401) == 5


def test_design_md_dispatch_table_is_the_plans():
    """DESIGN.md's dispatch table: every row's example shape takes the family, threads, points per thread and workgroups per
    scene the row states, and the rows reach every kernel the default build reaches."""
    text = open(os.path.join(REPO, "DESIGN.md")).read()
    rows = re.findall(r"^\|[^|\n]*\|[^|\n]*\| `fps_\w+` \((\w+)\) \| (\d+) \| (\d+) \| (\d+) \| \((\d+), (\d+), (\d+)\) \|$", text, flags=re.M)
    seen = set()
    for family, threads, ppt, G, B, N, M in rows:
        rc, p = cases.query_plan(int(B), int(N), int(M))
        assert rc == OK and (p["family"], p["threads"], p["ppt"], p["G"]) == (family, int(threads), int(ppt), int(G)), (N, M, p)
        seen.add(_key(p))
    assert seen == COMPILED - set(COMPILED_NOT_REACHED)
