"""The shapes at which the backwards (and forwards) of group_points / gather_knn / interpolate are tested, one table for
tests/test_scatter_route_cpu.py (does the library take the kernel each row names, and does the table reach every route, every
channels-per-workgroup value and both sides of every path boundary) and tests/test_gpu_gather_scatter_edges.py (the kernels at
these shapes in the three modes: default float32 atomics, deterministic float32, float64).

A row names, per mode, the route the library's own host functions report for it (``regnet_scatter_segsum_route`` for element
sizes 4 and 8, ``regnet_scatter_atomic_route``) -- never a copy of the thresholds:
    seg32 / seg64   (kind, channels): "one" = segsum_lds_kernel with every slot staged at once, "chunks" = the same kernel over
                    several chunks of slots, "global" = segsum_global_kernel
    atomic          (kind, channels): "lds" = scatter_add_lds_kernel, "global" = zero fill + group_bwd_kernel / interp_bwd_kernel
Shapes: group / knn  input (B, C, R), index (B, rows, K), gradient (B, C, rows, K), rows * K sources = slots per scene;
        interp       input (B, C, R), index / weight (B, rows, 3), gradient (B, C, rows), rows * 3 sources, rows slots.

Every index table carries, whatever the row is there for: the out-of-range values of ``bad_values`` (an index is compared as
int64: 2**32 + 5 is not destination 5), one destination that receives nothing (``empties``), destination 0 hit at regular
intervals (so in every chunk of a several-chunk route), the last destination and both ends of every 1024-destination scan round
hit at least once, a 64-source placement step on one destination and one on 64 distinct ones, and around every chunk edge of
either element size a run of sources on one destination (a segment that continues in the next chunk).  The three k of one
interpolate column share a slot (slot = position / 3), so they cannot lie on two sides of a chunk edge: the run there is the
two columns on either side of the edge, all six positions on one destination.
"""
import collections
import zlib

import numpy as np
import torch

SEG_KINDS = {0: None, 1: "one", 2: "chunks", 3: "global"}
ATOMIC_KINDS = {0: None, 1: "lds", 2: "global"}
OK, ERR_SHAPE, ERR_NULL, ERR_UNSUPPORTED = 0, -1, -2, -3

Case = collections.namedtuple("Case", "id op B C R rows K seg32 seg64 atomic tags")


def _g(id, B, C, R, rows, K, seg32, seg64, atomic, tags=()):
    return Case(id, "group", B, C, R, rows, K, seg32, seg64, atomic, frozenset(tags))


def _k(id, B, C, R, K, seg32, seg64, atomic, tags=()):          # gather_knn: as many index rows as points
    return Case(id, "knn", B, C, R, R, K, seg32, seg64, atomic, frozenset(tags))


def _i(id, B, C, R, rows, seg32, seg64, atomic, tags=()):
    return Case(id, "interp", B, C, R, rows, 3, seg32, seg64, atomic, frozenset(tags))


ONE1, CH1, LDS1 = ("one", 1), ("chunks", 1), ("lds", 1)
GL32, GL64, GLA = ("global", 4), ("global", 8), ("global", 16)

CASES = [
    # ---- one chunk | several chunks, in slots: 36 864 | 36 865 floats, 18 432 | 18 433 doubles ---------------------------------
    _g("g-slots-36864x1", 2, 3, 50, 36864, 1, ONE1, CH1, LDS1, {"boundary"}),
    _g("g-slots-36865x1", 2, 3, 50, 36865, 1, CH1, CH1, LDS1, {"boundary"}),
    _g("g-slots-576x64", 2, 2, 50, 576, 64, ONE1, CH1, LDS1, {"boundary"}),
    _g("g-slots-7373x5", 2, 3, 50, 7373, 5, CH1, CH1, LDS1, {"boundary"}),
    _g("g-slots-577x64", 1, 3, 50, 577, 64, CH1, CH1, LDS1, {"boundary"}),
    _g("g-slots-18432x1", 2, 3, 50, 18432, 1, ONE1, ONE1, LDS1, {"boundary"}),
    _g("g-slots-18433x1", 2, 3, 50, 18433, 1, ONE1, CH1, LDS1, {"boundary"}),
    _i("i-slots-36864", 2, 3, 50, 36864, ONE1, CH1, LDS1, {"boundary"}),
    _i("i-slots-36865", 2, 3, 50, 36865, CH1, CH1, LDS1, {"boundary"}),
    _i("i-slots-18432", 2, 2, 50, 18432, ONE1, ONE1, LDS1, {"boundary"}),
    _i("i-slots-18433", 2, 2, 50, 18433, ONE1, CH1, LDS1, {"boundary"}),
    # ---- several chunks | global kernel, in destinations: 16 384 | 16 385 (float), 9 557 | 9 558 (double) ----------------------
    _g("g-dest-16384", 2, 3, 16384, 7373, 5, CH1, GL64, LDS1, {"boundary"}),
    _g("g-dest-16385", 2, 5, 16385, 7373, 5, GL32, GL64, LDS1, {"boundary"}),
    _g("g-dest-9557", 2, 3, 9557, 18433, 1, ONE1, CH1, LDS1, {"boundary"}),
    _g("g-dest-9558", 2, 9, 9558, 18433, 1, ONE1, GL64, LDS1, {"boundary"}),
    _i("i-dest-16384", 2, 3, 16384, 36865, CH1, GL64, LDS1, {"boundary"}),
    _i("i-dest-16385", 2, 5, 16385, 36865, GL32, GL64, LDS1, {"boundary"}),
    _i("i-dest-9557", 2, 3, 9557, 18433, ONE1, CH1, LDS1, {"boundary"}),
    _i("i-dest-9558", 2, 9, 9558, 18433, ONE1, GL64, LDS1, {"boundary"}),
    # ---- LDS atomics | global atomics, in destinations: 36 864 | 36 865 ---------------------------------------------------------
    _g("g-atomic-36864", 2, 3, 36864, 600, 8, ONE1, ONE1, LDS1, {"boundary"}),
    _g("g-atomic-36865", 2, 17, 36865, 600, 8, ONE1, ONE1, GLA, {"boundary"}),
    _i("i-atomic-36864", 2, 3, 36864, 2000, ONE1, ONE1, LDS1, {"boundary"}),
    _i("i-atomic-36865", 2, 17, 36865, 2000, ONE1, ONE1, GLA, {"boundary"}),
    # ---- channels per workgroup, the last workgroup holding fewer ---------------------------------------------------------------
    _g("g-cpb8-last5", 8, 509, 40, 10, 6, ("one", 8), ("one", 8), ("lds", 8), {"cpb"}),
    _g("g-cpb4-last1", 8, 253, 40, 10, 6, ("one", 4), ("one", 4), ("lds", 4), {"cpb"}),
    _g("g-cpb2-last1", 8, 127, 40, 10, 6, ("one", 2), ("one", 2), ("lds", 2), {"cpb"}),
    _k("k-cpb4-last1", 8, 253, 40, 6, ("one", 4), ("one", 4), ("lds", 4), {"cpb"}),
    _i("i-cpb8-last5", 8, 509, 40, 20, ("one", 8), ("one", 8), ("lds", 8), {"cpb"}),
    _i("i-cpb2-last1", 8, 127, 40, 20, ("one", 2), ("one", 2), ("lds", 2), {"cpb"}),
    # 5 300 slots: 6 float rows fit, halved once (64 * ceil(23 / 6) < 512) = 3; 3 double rows fit
    _g("g-cpb3-last2", 64, 23, 40, 530, 10, ("one", 3), ("one", 3), ("lds", 2), {"cpb"}),
    # 4 700 slots: 7 float rows fit; 3 double rows
    _i("i-cpb7-last6", 64, 55, 40, 4700, ("one", 7), ("one", 3), ("lds", 4), {"cpb"}),
    # 2 400 slots: 7 double rows fit; 8 float rows, halved once
    _g("g-cpb7-f64-last6", 64, 55, 40, 240, 10, ("one", 4), ("one", 7), ("lds", 4), {"cpb"}),
    _g("g-cpb32-last31", 16, 1023, 40, 10, 6, ("one", 8), ("one", 8), ("lds", 32), {"cpb"}),
    _g("g-cpb16-last15", 16, 511, 40, 10, 6, ("one", 8), ("one", 8), ("lds", 16), {"cpb"}),
    _i("i-cpb32-last31", 16, 1023, 40, 20, ("one", 8), ("one", 8), ("lds", 32), {"cpb"}),
    # ---- plan edges: destinations around the scan round (1024) and the placement's key bits; sources mod 64 = 0, 1, 63 ---------
    _g("g-plan-R1", 2, 3, 1, 64, 4, ONE1, ONE1, LDS1, {"plan"}),                # 256 sources, nbits = 0
    _i("i-plan-R1", 2, 3, 1, 107, ONE1, ONE1, LDS1, {"plan"}),                  # 321
    _g("g-plan-R2", 2, 3, 2, 191, 1, ONE1, ONE1, LDS1, {"plan"}),               # 191 = 2 * 64 + 63
    _g("g-plan-R63", 2, 3, 63, 64, 5, ONE1, ONE1, LDS1, {"plan"}),              # 320
    _i("i-plan-R64", 2, 3, 64, 107, ONE1, ONE1, LDS1, {"plan"}),                # 321
    _k("k-plan-R65", 2, 3, 65, 5, ONE1, ONE1, LDS1, {"plan"}),                  # 325
    _g("g-plan-R65", 2, 3, 65, 383, 1, ONE1, ONE1, LDS1, {"plan"}),             # 383 = 5 * 64 + 63
    _i("i-plan-R1023", 2, 3, 1023, 1024, ONE1, ONE1, LDS1, {"plan"}),           # 3072
    _g("g-plan-R1024", 2, 3, 1024, 3073, 1, ONE1, ONE1, LDS1, {"plan"}),        # 3073 = 48 * 64 + 1
    _g("g-plan-R1025", 2, 3, 1025, 139, 29, ONE1, ONE1, LDS1, {"plan"}),        # 4031 = 62 * 64 + 63
    _i("i-plan-R2049", 2, 3, 2049, 2048, ONE1, ONE1, LDS1, {"plan"}),           # 6144
    _g("g-plan-R2049", 2, 3, 2049, 683, 9, ONE1, ONE1, LDS1, {"plan"}),         # 6147
]
BY_ID = {c.id: c for c in CASES}


def weighted(case):
    return case.op == "interp"


def num_src(case):
    """Sources per scene, as the segment sums count them (interpolate: rows * 3)."""
    return case.rows * case.K


def num_slots(case):
    return case.rows if weighted(case) else case.rows * case.K


def segsum_route(elem_size, is_weighted, B, C, R, L):
    """``regnet_scatter_segsum_route`` -> (status, (kind, channels, slots per chunk))."""
    import ctypes
    from regnet_for_3d_grasping_amd import _lib
    out = (ctypes.c_int64 * 3)()
    rc = _lib.call("regnet_scatter_segsum_route", None, elem_size, int(is_weighted), B, C, R, L, ctypes.addressof(out))
    return rc, (SEG_KINDS[int(out[0])], int(out[1]), int(out[2]))


def atomic_route(B, C, R, L):
    """``regnet_scatter_atomic_route`` -> (status, (kind, channels))."""
    import ctypes
    from regnet_for_3d_grasping_amd import _lib
    out = (ctypes.c_int64 * 2)()
    rc = _lib.call("regnet_scatter_atomic_route", None, B, C, R, L, ctypes.addressof(out))
    return rc, (ATOMIC_KINDS[int(out[0])], int(out[1]))


def routes(case):
    """The library's routes of a row: {"seg32": (kind, channels, chunk), "seg64": ..., "atomic": (kind, channels)}."""
    out = {}
    for name, size in (("seg32", 4), ("seg64", 8)):
        rc, out[name] = segsum_route(size, weighted(case), case.B, case.C, case.R, num_src(case))
        assert rc == OK, (case.id, name, rc)
    rc, out["atomic"] = atomic_route(case.B, case.C, case.R, case.rows if weighted(case) else num_src(case))
    assert rc == OK, (case.id, rc)
    return out


def chunk_edges(case):
    """The slots at which a chunk of either element size's several-chunk route begins (sorted, without slot 0)."""
    edges = set()
    r = routes(case)
    for name in ("seg32", "seg64"):
        kind, _, chunk = r[name]
        if kind == "chunks":
            edges.update(range(chunk, num_slots(case), chunk))
    return sorted(edges)


def bad_values(R):
    """Indices outside [0, R): both neighbours of the range, and values whose low 32 bits are a destination (5, 0)."""
    return [-1, R, 2 ** 32 + 5, -2 ** 32 + 5, 2 ** 40, 2 ** 32]


def empties(case):
    """Destinations no source points at (none where the 64 distinct destinations of a placement step need them all)."""
    R = case.R
    if R < 3 or 64 <= R < 128 or (R // 3) % 1024 in (0, 1023):
        return []
    return [R // 3]


def required(case):
    """Destinations with a non-zero count: the first and the last, and both ends of every 1024-destination scan round."""
    R = case.R
    req = {0, R - 1} | {n for n in range(R) if n % 1024 in (0, 1023)}
    return sorted(req - set(empties(case)))


def index(case):
    """-> int64 (B, rows, K), the same for every call."""
    rng = np.random.default_rng(zlib.crc32(case.id.encode()))
    B, R, L = case.B, case.R, num_src(case)
    per_slot = 3 if weighted(case) else 1
    idx = rng.integers(0, R, (B, L))
    free = np.ones(L, dtype=bool)        # positions no pattern below has taken

    def put(where, values):
        idx[:, where] = values
        free[where] = False

    if L >= 4096:
        put(slice(0, L, L // 48), 0)                               # destination 0 in every chunk
    req = np.array(required(case), dtype=np.int64)
    if L >= 192:
        assert L >= 192 + 2 * len(req) + 16, case.id
        put(slice(64, 128), R - 1)                                 # one placement step, one destination
        if R >= 64:
            put(slice(128, 192), R - 64 + np.arange(64))           # one placement step, 64 destinations
        put(slice(192, 192 + len(req)), req)
    else:
        assert L >= 4 * len(req), case.id
        put(slice(L - len(req), L), req)
    for e in chunk_edges(case):
        put(slice((e - 1) * per_slot - (per_slot == 1), (e + 1) * per_slot + (per_slot == 1)), R - 1)
    bad = np.array(bad_values(R), dtype=np.int64)
    for b in range(B):
        pos = rng.choice(np.flatnonzero(free), max(len(bad), L // 40), replace=False)
        idx[b, pos] = np.resize(bad, len(pos))
    for e in empties(case):
        idx[idx == e] = R + 1
    return torch.from_numpy(idx.reshape(B, case.rows, case.K))


def grad_shape(case):
    return (case.B, case.C, case.rows) if weighted(case) else (case.B, case.C, case.rows, case.K)


def _rng(case, salt):
    return np.random.default_rng([zlib.crc32(case.id.encode()), salt])


def mixed_grad(rng, shape):
    """float32 values of mixed magnitudes: sums of them depend on the order of the additions."""
    g = rng.standard_normal(shape) * np.exp2(rng.integers(-12, 12, shape))
    return torch.from_numpy(g.astype(np.float32))


def integer_values(rng, shape):
    """float32 integers in [-1024, 1024]."""
    return torch.from_numpy(rng.integers(-1024, 1025, shape).astype(np.float32))


def exact_inputs(case, idx):
    """-> (gradient, weight or None): integers in [-1024, 1024] and weights from {0, 0.25, 0.5, 1}.  Every product is then a
    multiple of 0.25 and so is every partial sum; a float32 holds every multiple of 0.25 below 2**22 (of 1 below 2**24), so
    with the sum of |g * w| of every destination below that the result does not depend on the order of the additions --
    asserted here."""
    rng = _rng(case, 1)
    g = integer_values(rng, grad_shape(case))
    w = None
    if weighted(case):
        w = torch.from_numpy(rng.choice(np.array([0, 0.25, 0.5, 1], dtype=np.float32), (case.B, case.rows, 3)))
    n, S = contributions(case, g.double(), idx, w.double() if w is not None else None)
    assert float(S.max()) < (2.0 ** 22 if w is not None else 2.0 ** 24), case.id
    return g, w


def rounded_inputs(case):
    """-> (gradient, weight or None): mixed magnitudes, Dirichlet weights."""
    rng = _rng(case, 2)
    g = mixed_grad(rng, grad_shape(case))
    w = torch.from_numpy(rng.dirichlet(np.ones(3), (case.B, case.rows)).astype(np.float32)) if weighted(case) else None
    return g, w


def forward_input(case, exact):
    rng = _rng(case, 3)
    shape = (case.B, case.C, case.R)
    return integer_values(rng, shape) if exact else mixed_grad(rng, shape)


def reference_backward(ref, case, g, idx, w):
    """The backward of the row's operator in ``ref`` (tests/f64_reference.py or tests/det_reference.py)."""
    if weighted(case):
        return ref.interpolate_backward(g, idx, w, case.R)
    if case.op == "knn":
        return ref.gather_knn_backward(g, idx)
    return ref.group_points_backward(g, idx, case.R)


def contributions(case, g64, idx, w64):
    """-> (n, S): per destination the number of in-range contributions (B, 1, R) and the float64 sum of |g * w| over them
    (B, C, R)."""
    from . import f64_reference as F
    ones = torch.ones((case.B, 1) + tuple(g64.shape[2:]), dtype=torch.float64)
    if weighted(case):
        return (F.interpolate_backward(ones, idx, torch.ones_like(w64), case.R),
                F.interpolate_backward(g64.abs(), idx, w64.abs(), case.R))
    return F.group_points_backward(ones, idx, case.R), F.group_points_backward(g64.abs(), idx, case.R)


U32 = 2.0 ** -24


def summation_bound(n, S):
    """The error bound of a float32 sum of n float32 products in any order against the exact sum: (n + 1) u S / (1 - (n + 1) u),
    u = 2**-24, S the sum of the products' magnitudes (Higham, Accuracy and Stability of Numerical Algorithms, section 4.2,
    with one more rounding for the product).  The float64 reference's own rounding is 2**-29 of it and less."""
    t = (n + 1.0) * U32
    return t * S / (1.0 - t)


def group_bound(g, idx, R):
    """summation_bound of ``group_points_backward(g, idx, R)`` -> (B, C, R) float64."""
    from . import f64_reference as F
    g64 = g.double().contiguous()
    ones = torch.ones((g.shape[0], 1) + tuple(g.shape[2:]), dtype=torch.float64)
    return summation_bound(F.group_points_backward(ones, idx, R), F.group_points_backward(g64.abs(), idx, R))


def interpolate_bound(g, idx, w, M):
    """summation_bound of ``interpolate_backward(g, idx, w, M)`` -> (B, C, M) float64."""
    from . import f64_reference as F
    g64, w64 = g.double().contiguous(), w.double()
    ones = torch.ones((g.shape[0], 1, g.shape[2]), dtype=torch.float64)
    return summation_bound(F.interpolate_backward(ones, idx, torch.ones_like(w64), M),
                           F.interpolate_backward(g64.abs(), idx, w64.abs(), M))


def strided(t, offset=7):
    """The values of ``t`` (B, C, ...) as the view the modules hand over -- channels last in memory, (B, ..., C) permuted -- at a
    non-zero storage offset, on the device of ``t``."""
    perm = (0,) + tuple(range(2, t.dim())) + (1,)
    back = (0, t.dim() - 1) + tuple(range(1, t.dim() - 1))
    buf = torch.empty(t.numel() + offset, dtype=t.dtype, device=t.device)
    rows = buf[offset:].view([t.shape[p] for p in perm])
    rows.copy_(t.permute(perm))
    out = rows.permute(back)
    assert out.shape == t.shape and out.storage_offset() == offset and out.stride(1) == 1
    return out
