"""The shapes at which furthest point sampling (csrc/geometry.hip, dispatched by ``fps_plan``) is tested, one table for
tests/test_fps_plan_cpu.py (does the library take the kernel each row is there for, and does the table reach every kernel the
dispatch can reach) and tests/test_gpu_ops.py (the kernels at these shapes, bit for bit against the CPU oracle).

``family`` and ``ppt`` of a row are what ``regnet_fps_plan`` reports for it: the kernel family and the points per thread
(0 for the streaming kernel, which keeps no point in a register).  Families, in the plan's numbering:
    1 resident   fps_resident_kernel<T, PPT>: points in registers, one pick per round
    2 cluster    fps_cluster_kernel<PPT, 8, false>: Morton-sorted, pruning per 64-point cluster, several picks per round
    3 sorted     fps_sorted_kernel<PPT, 4>: sorted, pruning per wave (more picks than the cluster kernel's LDS buffer holds)
    4 coop       fps_cluster_kernel<PPT, 8, true> on 2..4 cooperating workgroups per scene
    5 multi      fps_multi_kernel<25> on 2..4 cooperating workgroups per scene, one pick per round (M < 1024 or M > 8192)
    6 streaming  fps_streaming_kernel<1024>: running distances in the workspace
"""
import collections

FAMILIES = {1: "resident", 2: "cluster", 3: "sorted", 4: "coop", 5: "multi", 6: "streaming"}
PLAN_FIELDS = ("family", "threads", "ppt", "G", "Bpad", "grid", "workspace_bytes", "xchg_offset", "status_offset")
XCHG_BYTES, STATUS_BYTES = 2 * 4 * 64 * 8 * 4 + 256, 256   # per scene / per launch (include/regnet_hip.h: regnet_fps_plan)

Row = collections.namedtuple("Row", "B N M dup grid family ppt")
# a chain of three levels: M is (M1, M2, M3), family and ppt are level 1's (levels 2 and 3 sample M1 and M2 points)
Chain = collections.namedtuple("Chain", "B N M dup grid family ppt")


def shapes(rows):
    """The rows without their tags: what the GPU tests are parametrised with."""
    return [tuple(r[:5]) if r.dup is not None else tuple(r[:3]) for r in rows]


FPS_CASES = [  # (B, N, M, dup, grid)
    Row(2, 1024, 256, 0, None, "resident", 2), Row(2, 5120, 1024, 0, None, "cluster", 6),
    Row(1, 6144, 5120, 0, None, "cluster", 6), Row(2, 1, 1, 0, None, "resident", 1),
    Row(3, 20, 7, 0, None, "resident", 1), Row(1, 64, 64, 0, None, "resident", 1),
    Row(2, 300, 300, 0.3, None, "resident", 1), Row(2, 2048, 512, 0.5, None, "resident", 4),
    Row(2, 4096, 1024, 0, 0.05, "resident", 8), Row(1, 700, 200, 0, 0.1, "resident", 2),
    Row(1, 17, 17, 0.5, 0.2, "resident", 1), Row(1, 9000, 700, 0.2, 0.02, "resident", 12),
    Row(1, 13000, 300, 0, None, "resident", 16), Row(1, 20000, 300, 0.1, None, "resident", 20),
    # N > 8192: heavy ties / duplicates / degenerate extents, on whichever kernel the run length selects
    Row(1, 12000, 2000, 0.3, 0.05, "cluster", 12), Row(2, 25600, 1000, 0.5, 0.01, "resident", 25),
    Row(1, 9000, 9000, 0.1, None, "sorted", 12), Row(1, 16000, 500, 0.9, 0.1, "resident", 16),
    # the resident (threads, points per thread) pairs nothing above reaches: N just above a threshold, short runs
    Row(1, 65, 33, 0, None, "resident", 1), Row(1, 4097, 300, 0, None, "resident", 6), Row(1, 6145, 511, 0.1, 0.03, "resident", 8),
]

FPS_CLUSTER_CASES = [  # (B, N, M, dup, grid): long runs = the sorting kernels (several exact picks per round, csrc/geometry.hip)
    Row(2, 25600, 1500, 0.5, 0.01, "cluster", 25),   # heavy duplicates + lattice ties: the exact one-pick path in between batched rounds
    Row(1, 10000, 1024, 0, 0.2, "cluster", 12),      # 125 distinct points, 1024 picks: all distances zero after 125 -> the reference repeats its pick
    Row(1, 12001, 1100, 0.1, None, "cluster", 12),   # N not a multiple of the 64-point cluster
    Row(1, 8193, 1024, 0, None, "cluster", 12), Row(1, 4097, 512, 0.2, 0.03, "cluster", 6), Row(2, 8192, 2048, 0, None, "cluster", 8),
    Row(1, 16000, 1200, 0, None, "cluster", 16), Row(1, 20000, 8192, 0.05, None, "cluster", 20),   # 16 / 20 slots per lane; M at the LDS pick buffer's capacity
    Row(1, 20480, 8193, 0, None, "sorted", 20),      # one more: the per-wave kernel (fps_sorted_kernel<20, 4>) takes over
    Row(3, 25600, 5120, 0, None, "cluster", 25),
    # the per-wave kernel at 16 and 25 points per thread: the smallest N of each bracket, one pick beyond the LDS buffer
    Row(1, 12289, 8193, 0, None, "sorted", 16), Row(1, 20481, 8193, 0, None, "sorted", 25),
]

FPS_MULTI_CASES = [Row(1, 30000, 200, None, None, "multi", 25), Row(3, 51200, 700, None, None, "multi", 25),
                   Row(2, 60000, 300, None, None, "multi", 25), Row(1, 102400, 150, None, None, "multi", 25)]

FPS_COOP_CASES = [Row(2, 51200, 5120, 0, None, "coop", 25), Row(1, 30000, 1500, 0.2, None, "coop", 16),
                  Row(1, 76800, 2048, 0, None, "coop", 25), Row(1, 102400, 1024, 0, None, "coop", 25),
                  Row(2, 40000, 1200, 0.4, 0.02, "coop", 20), Row(1, 25601, 1024, 0, None, "coop", 16),
                  Row(1, 50000, 1300, 0, 0.25, "coop", 25)]

CHAIN_CASES = [  # (B, N, (M1, M2, M3), dup, grid)
    Chain(3, 25600, (5120, 1024, 256), 0.0, None, "cluster", 25),      # the network's three levels on generic clouds
    Chain(2, 51200, (5120, 1024, 256), 0.0, None, "coop", 25),         # level 1 on cooperating workgroups
    Chain(2, 6144, (5120, 1024, 256), 0.0, None, "cluster", 6),        # the small golden configuration
    Chain(2, 25600, (5120, 1024, 256), 0.3, None, "cluster", 25),      # duplicated points: zero distances and exact ties
    Chain(2, 12000, (4096, 1024, 256), 0.0, 0.05, "cluster", 12),      # lattice: ties at the maximum are frequent
    Chain(1, 30000, (2048, 1024, 300), 0.1, 0.02, "coop", 16),         # cooperative + lattice + duplicates
    Chain(2, 3000, (1024, 512, 64), 0.0, None, "resident", 8),         # level 1 on a kernel that does not track ties ("unknown")
    Chain(1, 9000, (8800, 8000, 3000), 0.0, None, "sorted", 12),       # nearly every point picked, long chains
]

# the shapes of the tests that build their own cloud (dup / grid: not `cloud()`'s)
SINGLE = {
    "flat_plane_and_line_long_run": Row(1, 14000, 1500, None, None, "cluster", 16),
    "zero_extent_long_run": Row(1, 9000, 1024, None, None, "cluster", 12),
    "many_equal_maxima": Row(1, 6 * 1728, 1500, None, None, "cluster", 12),
    "identical_small": Row(2, 130, 40, None, None, "resident", 1),
    "identical_zero_extent": Row(1, 10000, 50, None, None, "resident", 12),
    "planar_and_collinear_short_run": Row(1, 11000, 800, None, None, "resident", 12),
    "full_size": Row(2, 25600, 5120, None, None, "cluster", 25),
    "status_word": Row(2, 51200, 1024, None, None, "coop", 25),
    "multi_ties_and_duplicates": Row(1, 36000, 400, None, None, "multi", 25),
    "streaming": Row(1, 33500, 33000, None, None, "streaming", 0),
    "small_scenes_under_load": Row(96, 1024, 256, None, None, "resident", 2),
}


def all_rows():
    """Every (B, N, M) the GPU tests sample, with the tags of its row; the lower levels of the chains are not tagged."""
    rows = FPS_CASES + FPS_CLUSTER_CASES + FPS_MULTI_CASES + FPS_COOP_CASES + list(SINGLE.values())
    return rows + [Row(c.B, c.N, c.M[0], c.dup, c.grid, c.family, c.ppt) for c in CHAIN_CASES]


def query_plan(B, N, M):
    """``regnet_fps_plan`` -> (status, dict of its nine outputs, the family by name)."""
    import ctypes
    from regnet_for_3d_grasping_amd import _lib
    out = (ctypes.c_int64 * len(PLAN_FIELDS))()
    rc = _lib.call("regnet_fps_plan", None, B, N, M, ctypes.addressof(out))
    plan = dict(zip(PLAN_FIELDS, [int(v) for v in out]))
    plan["family"] = FAMILIES.get(plan["family"])
    return rc, plan
