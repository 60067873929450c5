"""The region-grouping kernels (csrc/region.hip through region_ops) on the MI355X at the shapes and values where they can go
wrong unnoticed: clouds that fill no wave quarter, groups that fill no chunk, points exactly on a membership boundary, a
candidate capacity below the member count, ids out of range, ties between rows.  Against the numpy restatement of the contract
(tests/region_reference.py), whose input builders tests/test_region_reference_cpu.py has shown to contain those cases.
Every comparison is exact, except the float32 row sums of random numbers (their bound is derived in ``ref.rowsum_bound``)."""
import numpy as np
import pytest
import torch

from . import region_reference as ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL = -7


@pytest.fixture(scope="module")
def ops():
    from regnet_for_3d_grasping_amd import region_ops
    return region_ops


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def cut(x, axis):
    """The values of ``x`` (numpy) as a device view cut out of a larger tensor: every second entry along axis 0 and, for axis
    1, behind three rows of padding -- so the stride of axis 0 is not the product of the other sizes."""
    shape = list(x.shape)
    shape[0] = 2 * shape[0] + 1
    if axis == 1:
        shape[1] += 3
    big = torch.full(shape, 7.0, dtype=torch.float32, device=DEV)
    view = big[1::2, 3:] if axis == 1 else big[1::2]
    view.copy_(torch.from_numpy(x))
    assert view.shape == x.shape and view.stride(-1) == 1 and view.stride(0) != int(np.prod(x.shape[1:]))
    return view


def assert_lists_equal(cand, count, want_cand, want_count):
    """counts equal and the first ``count`` entries of every list equal."""
    cand, count = cand.cpu().numpy(), count.cpu().numpy()
    assert cand.dtype == np.int32 and count.dtype == np.int32
    assert cand.shape == want_cand.shape and np.array_equal(count, want_count)
    valid = np.arange(want_cand.shape[-1]) < want_count[..., None]
    assert np.array_equal(cand[valid], want_cand[valid])


# ---- radius grouping -------------------------------------------------------------------------------------------------------
def radius_on_device(ops, pc, centres, radius):
    """6-channel cloud as a strided batch slice, centres as the [:, :, :3] view of 6-channel rows."""
    return ops.radius_candidates(cut(pc, 1), cut(centres, 0)[:, :, :3], radius)


@pytest.mark.parametrize("layout", ref.RADIUS_LAYOUTS)
def test_radius_candidates_ragged_clouds(ops, layout):
    for N in ref.RADIUS_N:
        for B in (1, 3):
            for Nc in (1, 5):
                pc, centres, r = ref.radius_case(layout, B, N, Nc, seed=N + Nc)
                want = ref.radius_candidates(pc, centres, ops.sqrt_le_threshold(r))
                assert_lists_equal(*radius_on_device(ops, pc, centres, r), *want)


def test_radius_candidates_empty_cloud(ops):
    pc = torch.zeros((2, 0, 6), dtype=torch.float32, device=DEV)
    centres = torch.zeros((2, 3, 6), dtype=torch.float32, device=DEV)
    cand, count = ops.radius_candidates(pc, centres[:, :, :3], 0.05)
    assert cand.shape == (2, 3, 1) and count.cpu().tolist() == [[0, 0, 0]] * 2


@pytest.mark.parametrize("radius", ref.BOUNDARY_RADII)
def test_radius_is_inclusive_to_the_last_float(ops, radius):
    pc, centres, r = ref.radius_boundary_case(radius)
    want = ref.radius_candidates(pc, centres, ops.sqrt_le_threshold(r))
    assert_lists_equal(*radius_on_device(ops, pc, centres, r), *want)


@pytest.mark.parametrize("cap", ref.CAPACITIES)
def test_radius_group_capacity_below_the_count(ops, cap):
    """The C entry point with cap < count: the full count is reported, the first ``cap`` members are written and nothing
    else is touched -- neither the rest of a shorter list nor the words behind the last list."""
    from regnet_for_3d_grasping_amd import _lib
    pc, centres, r = ref.capacity_case(3)
    B, N, _ = pc.shape
    Nc = centres.shape[1]
    T = ops.sqrt_le_threshold(r)
    want_cand, want_count = ref.radius_candidates(pc, centres, T)
    p, c = dev(pc), dev(centres)
    buf = torch.full((B * Nc * cap + 64,), SENTINEL, dtype=torch.int32, device=DEV)
    count = torch.full((B, Nc), SENTINEL, dtype=torch.int32, device=DEV)
    status = _lib.lib.regnet_radius_group_f32(p.data_ptr(), N * 6, 6, c.data_ptr(), Nc * 6, 6, B, N, Nc, T, cap,
                                              buf.data_ptr() if cap else None, count.data_ptr(),
                                              torch.cuda.current_stream(p.device).cuda_stream)
    assert status == 0
    assert np.array_equal(count.cpu().numpy(), want_count)
    buf = buf.cpu().numpy()
    assert (buf[B * Nc * cap:] == SENTINEL).all()
    lists = buf[:B * Nc * cap].reshape(B, Nc, cap)
    for b in range(B):
        for k in range(Nc):
            n = min(int(want_count[b, k]), cap)
            assert np.array_equal(lists[b, k, :n], want_cand[b, k, :n])
            assert (lists[b, k, n:] == SENTINEL).all()


# ---- box crop --------------------------------------------------------------------------------------------------------------
def box_on_device(ops, pts, centre, rot, xl, yl, zl):
    return ops.box_candidates(cut(pts, 0), dev(centre), dev(rot), dev(xl), dev(yl), zl)


@pytest.mark.parametrize("kind", ["random", "inside", "outside"])
def test_box_candidates_ragged_groups(ops, kind):
    for n in ref.BOX_N:
        for G in ref.BOX_G:
            case = ref.box_case(kind, n, G, seed=n * 1000 + G)
            want_cand, want_count = ref.box_candidates(*case)
            cand, count = box_on_device(ops, *case)
            assert_lists_equal(cand, count, want_cand, want_count)
            if kind != "random":
                assert count.cpu().tolist() == [G if kind == "inside" else 0] * n


def test_box_faces_are_strict(ops):
    pts, centre, rot, xl, yl, zl, inside = ref.box_strict_case()
    cand, count = box_on_device(ops, pts, centre, rot, xl, yl, zl)
    cand, count = cand.cpu().numpy(), count.cpu().numpy()
    for i in range(len(inside)):
        assert cand[i, :count[i]].tolist() == np.nonzero(inside[i])[0].tolist(), i


# ---- resample --------------------------------------------------------------------------------------------------------------
@pytest.fixture
def range_flag(ops):
    """The out-of-range flag is lowered before the test and after it, whatever the test did."""
    def lower():
        try:
            ops.raise_if_out_of_range()
        except RuntimeError:
            pass
    lower()
    try:
        yield
    finally:
        lower()


def resample_on_device(ops, pc, cand, pos):
    index, points = ops.resample_groups(cut(pc, 1), dev(cand), dev(pos))
    assert index.dtype == torch.int64 and points.dtype == torch.float32
    return index.cpu().numpy(), points.cpu().numpy()


@pytest.mark.parametrize("C", ref.RESAMPLE_C)
def test_resample_groups_ragged(ops, range_flag, C):
    for B, Nc, G in ref.RESAMPLE_SHAPES:
        pc, cand, pos = ref.resample_case(B, Nc, G, C, seed=C + G)
        want_index, want_points, flag = ref.resample_groups(pc, cand, pos)
        index, points = resample_on_device(ops, pc, cand, pos)
        assert not flag and np.array_equal(index, want_index) and np.array_equal(points, want_points)
    ops.raise_if_out_of_range()          # nothing was out of range: does not raise


def test_resample_groups_rejects_65_channels(ops, range_flag):
    pc, cand, pos = ref.resample_case(1, 2, 3, 65, seed=0)
    with pytest.raises(RuntimeError, match="resample_groups"):
        ops.resample_groups(dev(pc), dev(cand), dev(pos))


@pytest.mark.parametrize("what", ["position_at_capacity", "candidate_at_cloud_size"])
def test_resample_groups_out_of_range_is_flagged_once(ops, range_flag, what):
    B, Nc, G, C = 2, 5, 37, 6
    pc, cand, pos = ref.resample_case(B, Nc, G, C, seed=9)
    if what == "position_at_capacity":
        pos[1, 2, 5] = cand.shape[2]
    else:
        cand[0, 3, pos[0, 3, 11]] = pc.shape[1]
    want_index, want_points, flag = ref.resample_groups(pc, cand, pos)
    assert flag and 0 < (want_index[pos >= 0] < 0).sum() < G
    index, points = resample_on_device(ops, pc, cand, pos)
    assert np.array_equal(index, want_index) and np.array_equal(points, want_points)
    assert (points[index < 0] == -1.0).all()
    with pytest.raises(RuntimeError, match="out of range"):
        ops.raise_if_out_of_range()
    ops.raise_if_out_of_range()          # the flag was lowered by the first call


# ---- gather + max ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F", ref.GATHER_F_V4 + ref.GATHER_F_SCALAR)
def test_gather_max_group_tails_and_skipped_ids(ops, F):
    for G in ref.GATHER_G:
        for R in ref.GATHER_R:
            for seed in (0, 1):
                feat, rows = ref.gather_case(F, G, R, seed)
                f = dev(feat)
                assert f.data_ptr() % 16 == 0
                got = ops.gather_max(f, dev(rows))
                assert got.shape == (R, F) and np.array_equal(got.cpu().numpy(), ref.gather_max(feat, rows)), (G, R, seed)


def test_gather_max_all_skipped_group_is_minus_infinity_on_both_paths(ops):
    for F in (256, 257):
        feat, _ = ref.gather_case(F, 17, 1, 0)
        rows = np.array([[-1, 37, -40, 99] + [-3] * 13, [5] * 17], dtype=np.int64)
        got = ops.gather_max(dev(feat), dev(rows)).cpu().numpy()
        assert np.isneginf(got[0]).all() and np.array_equal(got[1], feat[5])


def test_gather_max_unaligned_rows_take_the_scalar_kernel_same_bits(ops):
    F = 256
    for G in ref.GATHER_G:
        feat, rows = ref.gather_case(F, G, 5, seed=G)
        aligned = dev(feat)
        store = torch.empty((feat.size + 4,), dtype=torch.float32, device=DEV)
        shifted = store[1:1 + feat.size].view(feat.shape)
        shifted.copy_(aligned)
        assert aligned.data_ptr() % 16 == 0 and shifted.data_ptr() % 16 == 4 and shifted.is_contiguous()
        r = dev(rows)
        v4, scalar = ops.gather_max(aligned, r), ops.gather_max(shifted, r)
        assert torch.equal(v4, scalar)
        assert np.array_equal(v4.cpu().numpy(), ref.gather_max(feat, rows))


@pytest.mark.parametrize("F", (4, 256, 260))
def test_gather_max_scene_subset_of_lists(ops, F):
    for G in ref.GATHER_G:
        feat, index, row_ids, per_scene, stride = ref.scene_case(F, G, seed=G)
        f, i = dev(feat), dev(index)
        got = ops.gather_max_scene(f, i, dev(row_ids), per_scene, stride).cpu().numpy()
        assert np.array_equal(got, ref.gather_max(feat, index, row_ids=row_ids, per_scene=per_scene, scene_stride=stride)), G
        got = ops.gather_max_scene(f, i, None, per_scene, stride).cpu().numpy()
        assert np.array_equal(got, ref.gather_max(feat, index, per_scene=per_scene, scene_stride=stride)), G


# ---- gather_max_arg + scatter_max_grad -------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ref.ARG_SHAPES)
def test_gather_max_arg_first_maximum_wins_and_scatter_is_exact(ops, shape):
    F, G, R = shape
    feat, rows, dy, B, N = ref.arg_case(F, G, R, seed=F + G)
    num_rows = B * N
    want_out, want_arg = ref.gather_max_arg(feat, rows)
    out, arg = ops._gather_max_arg(dev(feat), dev(rows))
    assert arg.dtype == torch.int64
    assert np.array_equal(out.cpu().numpy(), want_out)
    assert np.array_equal(arg.cpu().numpy(), want_arg)
    # dy holds whole numbers in [-4, 4] and R <= 64: every float32 partial sum is exact in any order of the atomics
    d = dev(dy)
    grad = torch.zeros((num_rows, F), dtype=torch.float32, device=DEV)
    ops._scatter_max_grad(d, arg, grad, num_rows, 0, F, 1)
    assert np.array_equal(grad.cpu().numpy().astype(np.float64), ref.scatter_max_grad(dy, want_arg, (num_rows, F), num_rows, 0, F, 1))
    grad = torch.zeros((B, F, N), dtype=torch.float32, device=DEV)
    ops._scatter_max_grad(d, arg, grad, N, F * N, 1, N)
    assert np.array_equal(grad.cpu().numpy().astype(np.float64), ref.scatter_max_grad(dy, want_arg, (B, F, N), N, F * N, 1, N))


# ---- rowsum_neg ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", ref.ROWSUM_K)
def test_rowsum_neg(ops, K):
    for rows in ref.ROWSUM_ROWS:
        x = ref.rowsum_case("integer", rows, K, seed=rows + K)
        got = ops.rowsum_neg(dev(x), K)
        assert got.shape == (rows,) and np.array_equal(got.cpu().numpy().astype(np.float64), ref.rowsum_neg(x)), rows
        x = ref.rowsum_case("randn", rows, K, seed=rows + K)
        got = ops.rowsum_neg(dev(x), K).cpu().numpy().astype(np.float64)
        err, bound = np.abs(got - ref.rowsum_neg(x)), ref.rowsum_bound(x)
        print("rowsum_neg K %d rows %d: max err / bound %.3f" % (K, rows, float((err / bound).max())))
        assert (err <= bound).all(), rows
    # the same through a leading shape, as the trainer calls it: (a, b, K) -> (a, b)
    x = ref.rowsum_case("integer", 6 * 11, K, seed=K).reshape(6, 11, K)
    assert np.array_equal(ops.rowsum_neg(dev(x), K).cpu().numpy().astype(np.float64), ref.rowsum_neg(x))


def test_rowsum_neg_rejects_what_it_cannot_do(ops):
    for K in (12, 512):
        with pytest.raises(RuntimeError, match="rowsum_neg"):
            ops.rowsum_neg(torch.zeros((8, K), dtype=torch.float32, device=DEV), K)
    store = torch.zeros((8 * 16 + 4,), dtype=torch.float32, device=DEV)
    shifted = store[1:1 + 8 * 16].view(8, 16)
    assert shifted.data_ptr() % 16 == 4 and shifted.is_contiguous()
    with pytest.raises(RuntimeError, match="rowsum_neg"):
        ops.rowsum_neg(shifted, 16)
