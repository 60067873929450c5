"""``pn2_ext`` for MI355X: the reference's seven pybind entry points
(multi_model/utils/pn2_utils/csrc/main.cpp:6-14) on top of libregnet_hip.so.

Same names, argument order, shapes, dtypes and error behaviour as the CUDA extension:
inputs must be GPU tensors (the reference's CHECK_CUDA -- there is no CPU path), may be
non-contiguous views, are never modified; outputs are freshly allocated; failed checks raise
RuntimeError.  Kernels are enqueued on torch's current stream of the input's device.

dtypes: float32 or float64, like the reference's AT_DISPATCH_FLOATING_TYPES.  float32 runs the tuned kernels
(csrc/geometry.hip, grid.hip, gather.hip); float64 runs the forwards of csrc/ops_f64.hip (same semantics) and the
deterministic backwards of csrc/scatter.hip (see include/regnet_hip.h).  All float inputs of one call share one dtype
(mixing raises, as the reference's ``data<scalar_t>()`` does); float outputs take it, index / count outputs are int64.

Under ``torch.use_deterministic_algorithms(True)`` the float32 backwards follow the float64 ones' contract in float32
(each destination adds its contributions in ascending source position from +0.0; see determinism.py): the same plan and
segment-sum kernels of csrc/scatter.hip, instantiated for float.
"""
import torch

from . import _lib, determinism

_call = _lib.call
_L = _lib.lib

# Source clouds with at least this many points are binned into a uniform grid first (csrc/grid.hip);
# smaller ones are cheaper to scan exhaustively from LDS.  Results are identical either way.
GRID_MIN_POINTS = 2048        # 3-NN keys
GRID_MIN_POINTS_BALL = 8192   # ball-query cloud (measured break-even between 5 120 and 25 600 points)


def _need_gpu(t, name):
    if not isinstance(t, torch.Tensor):
        raise TypeError("%s must be a torch.Tensor" % name)
    if not t.is_cuda:
        raise RuntimeError("%s must be a CUDA tensor" % name)  # CHECK_CUDA (sampling_kernel.cu:11)


def _need_f32(t, name):
    _need_gpu(t, name)
    if t.dtype != torch.float32:
        raise RuntimeError("%s must be float32 (REGNet's path is fp32 only)" % name)


def _need_float(t, name, like=None):
    """float32 or float64 GPU tensor (the reference's AT_DISPATCH_FLOATING_TYPES), of the dtype of ``like`` when given.
    -> True for float64."""
    _need_gpu(t, name)
    if t.dtype not in (torch.float32, torch.float64):
        raise RuntimeError("%s must be float32 or float64" % name)
    if like is not None and t.dtype != like.dtype:
        raise RuntimeError("%s is %s but the other float inputs are %s" % (name, t.dtype, like.dtype))
    return t.dtype == torch.float64


def _entry(name, x):
    """The name of the entry point ``regnet_<name>_f64`` or ``_f32``, by the dtype of ``x``."""
    return "regnet_%s_%s" % (name, "f64" if x.dtype == torch.float64 else "f32")


def _need_i64(t, name):
    _need_gpu(t, name)
    if t.dtype != torch.int64:
        raise RuntimeError("%s must be int64" % name)


def _eq(a, b, text):
    if a != b:
        raise RuntimeError("%s" % text)  # CHECK_EQ


class FpsChain:
    """Optional third argument of ``farthest_point_sample`` for callers that sample a cloud which is itself a
    furthest-point-sampling sequence (PointNet++ levels 2 and 3 sample the previous level's centroids in pick order):
    ``prefix_ok`` in -- the ``first_tie`` tensor of the run that produced the cloud's order, or None -- and ``first_tie``
    out, (B,) int32 (include/regnet_hip.h: regnet_fps_chain_f32).  Scenes whose producing run had no tie among its first M
    picks get 0 .. M-1 without sampling; the result is the same tensor either way."""

    def __init__(self, prefix_ok=None):
        self.prefix_ok, self.first_tie = prefix_ok, None


def farthest_point_sample(points, num_centroids, chain=None):
    """points (B,3,N1) -> index (B,N2) int64.  csrc/sampling_kernel.cu:126-170.  ``chain``: see FpsChain (not part of the
    reference's signature; the result does not depend on it; float32 only)."""
    f64 = _need_float(points, "points")
    _eq(points.dim(), 3, "points must be (B, 3, N)")
    _eq(points.size(1), 3, "points.size(1) does not equal to 3")
    B, _, N = points.shape
    M = int(num_centroids)
    if not M > 0:
        raise RuntimeError("num_centroids is not greater than 0")
    if not N >= M:
        raise RuntimeError("num_points is less than num_centroids")
    if f64 and chain is not None:
        raise RuntimeError("FpsChain is a float32 mechanism; float64 points take no chain")
    index = torch.empty((B, M), dtype=torch.int64, device=points.device)
    ws_bytes = (_L.regnet_fps_f64_workspace_bytes if f64 else _L.regnet_fps_workspace_bytes)(B, N, M)
    ws = torch.empty((ws_bytes // points.element_size(),), dtype=points.dtype, device=points.device) \
        if ws_bytes else None
    sb, sc, sn = points.stride()
    if chain is None:
        _call(_entry("fps", points), points, points.data_ptr(), sb, sc, sn, B, N, M, index.data_ptr(),
              ws.data_ptr() if ws is not None else None)
    else:
        prefix = chain.prefix_ok
        if prefix is not None and (prefix.dtype != torch.int32 or prefix.numel() != B or not prefix.is_cuda):
            raise RuntimeError("FpsChain.prefix_ok must be a (B,) int32 GPU tensor")
        prefix = prefix.contiguous() if prefix is not None else None   # held across the call
        chain.first_tie = torch.empty((B,), dtype=torch.int32, device=points.device)
        _call("regnet_fps_chain_f32", points, points.data_ptr(), sb, sc, sn, B, N, M, index.data_ptr(),
              ws.data_ptr() if ws is not None else None, prefix.data_ptr() if prefix is not None else None,
              chain.first_tie.data_ptr())
    status_at = -1 if f64 else _L.regnet_fps_status_offset_bytes(B, N, M)
    if status_at >= 0:
        # cooperative sampling (N > 25 600): accumulate the launch's status word into the device's flag -- one tiny
        # launch on the same stream, no synchronisation; raise_if_fps_failed() reads it where the caller synchronises
        flag = _fps_flag(points.device)
        torch.bitwise_or(flag, ws[status_at // 4: status_at // 4 + 1].view(torch.int32), out=flag)
    return index


def gather_points(points, index, channels_last=False):
    """points (B,C,N) float32, index (B,M) int64 -> (B,C,M): ``points[b, :, index[b, m]]`` (pn2_utils/function.py:11-26's
    ``torch.gather``) as one native launch; any strides.  ``channels_last``: the result as a contiguous (B,M,C) tensor (rows of
    a (B,N,C) cloud handed in as its transposed view).  An index outside [0, N) flags the device's status word
    (``raise_if_fps_failed`` reports it where the caller synchronises) and yields 0."""
    _need_f32(points, "points")
    _need_i64(index, "index")
    _eq(points.dim(), 3, "points must be (B, C, N)")
    _eq(index.dim(), 2, "index must be (B, M)")
    _eq(points.size(0), index.size(0), "points and index differ in batch size")
    B, C, N = points.shape
    M = index.size(1)
    if channels_last:
        out = torch.empty((B, M, C), dtype=torch.float32, device=points.device)
        ob, om, oc = out.stride()
    else:
        out = torch.empty((B, C, M), dtype=torch.float32, device=points.device)
        ob, oc, om = out.stride()
    _call("regnet_gather_points_f32", points, points.data_ptr(), *points.stride(), B, C, N, index.data_ptr(), *index.stride(),
          M, out.data_ptr(), ob, oc, om, _fps_flag(points.device).data_ptr())
    return out


def class_order(count):
    """count (...) int64 GPU tensor of ball-query member counts -> (count.numel(),) int64: the stable sort permutation by cost
    class (count > 32) + (count > 48) (``torch.argsort(cls, stable=True)``), one launch (regnet_class_order_i64)."""
    _need_i64(count, "count")
    flat = count.reshape(-1)
    flat = flat if flat.is_contiguous() else flat.contiguous()
    order = torch.empty((flat.numel(),), dtype=torch.int64, device=count.device)
    _call("regnet_class_order_i64", count, flat.data_ptr(), flat.numel(), order.data_ptr())
    return order


def pair_order(count):
    """count (...) int64 GPU tensor of ball-query member counts -> (count.numel(),) int64: the processing order that puts
    neighbourhoods whose remainders share a point tile at slots 8 g + w and 8 g + w + 4, pairs sorted by cost in tiles
    (regnet_pair_order_i64, one launch; ``fused.chain3_pair_order`` states the same plan in numpy)."""
    _need_i64(count, "count")
    flat = count.reshape(-1)
    flat = flat if flat.is_contiguous() else flat.contiguous()
    order = torch.empty((flat.numel(),), dtype=torch.int64, device=count.device)
    work = torch.empty((flat.numel(),), dtype=torch.int32, device=count.device)
    _call("regnet_pair_order_i64", count, flat.data_ptr(), flat.numel(), order.data_ptr(), work.data_ptr())
    return order


_fps_flags = {}


def _fps_flag(device):
    key = (device.type, device.index if device.index is not None else torch.cuda.current_device())
    if key not in _fps_flags:
        _fps_flags[key] = torch.zeros(1, dtype=torch.int32, device=device)
    return _fps_flags[key]


def raise_if_fps_failed():
    """RuntimeError if a cooperative furthest-point-sampling launch since the last check lost a partner workgroup (a
    scene's 2-4 workgroups exchange records every round and must all be resident; a poll gives up after 2^22 tries, flags
    the launch and stops instead of sampling on with diverged selections).  Synchronises; called where the caller
    synchronises anyway (end of pipeline.forward_scenes / ForwardPipeline.run), like region_ops.raise_if_out_of_range."""
    for flag in _fps_flags.values():
        if int(flag.item()):
            flag.zero_()
            raise RuntimeError("farthest_point_sample: a cooperating workgroup lost its partner (launch not fully "
                               "resident?) -- the returned indices are incomplete -- or gather_points saw an index "
                               "outside the cloud")


def ball_query(points, centroids, radius, num_neighbours):
    """points (B,3,N1), centroids (B,3,N2) -> [index (B,N2,K) int64, count (B,N2) int64].
    csrc/ball_query_kernel.cu:87-131."""
    f64 = _need_float(points, "points")
    _need_float(centroids, "centroids", points)
    _eq(points.size(1), 3, "points.size(1) does not equal to 3")
    _eq(centroids.size(1), 3, "centroids.size(1) does not equal to 3")
    _eq(centroids.size(0), points.size(0), "centroids.size(0) does not equal to batch_size")
    B, _, N1 = points.shape
    N2 = centroids.size(2)
    K = int(num_neighbours)
    index = torch.empty((B, N2, K), dtype=torch.int64, device=points.device)
    count = torch.empty((B, N2), dtype=torch.int64, device=points.device)
    if not f64 and N1 >= GRID_MIN_POINTS_BALL and K <= 64 and B > 0 and float(radius) > 0:
        ws = torch.empty((_L.regnet_grid_workspace_bytes(B, N1),), dtype=torch.uint8, device=points.device)
        _call("regnet_ball_query_grid_f32", points, points.data_ptr(), *points.stride(), centroids.data_ptr(),
              *centroids.stride(), B, N1, N2, float(radius), K, index.data_ptr(), count.data_ptr(), ws.data_ptr())
    else:
        _call(_entry("ball_query", points), points, points.data_ptr(), *points.stride(), centroids.data_ptr(),
              *centroids.stride(), B, N1, N2, float(radius), K, index.data_ptr(), count.data_ptr())
    return [index, count]


def group_points_forward(input, index):
    """input (B,C,N1), index (B,N2,K) -> (B,C,N2,K).  csrc/grouping_kernel.cu:29-51."""
    _need_float(input, "input")
    _need_i64(index, "index")
    _eq(input.dim(), 3, "input.dim() does not equal to 3")
    _eq(index.dim(), 3, "index.dim() does not equal to 3")
    _eq(index.size(0), input.size(0), "index.size(0) does not equal to batch_size")
    B, C, N1 = input.shape
    _, N2, K = index.shape
    idx = index.contiguous()
    out = torch.empty((B, C, N2, K), dtype=input.dtype, device=input.device)
    _call(_entry("group_points_fwd", input), input, input.data_ptr(), *input.stride(), idx.data_ptr(), B, C, N1, N2, K,
          out.data_ptr())
    return out


def group_points_backward(grad_output, index, num_points, plan=None):
    """grad_output (B,C,N2,K), index (B,N2,K) -> grad_input (B,C,N1).  csrc/grouping_kernel.cu:103-149.  float64, and
    float32 in deterministic mode: summed in ascending (n2, k) order per destination, run to run bit-identical.
    ``plan``: ``scatter_plan(index, num_points)`` when the caller already has it (deterministic mode; else built here)."""
    _need_float(grad_output, "grad_output")
    _need_i64(index, "index")
    _eq(grad_output.dim(), 4, "grad_output.dim() does not equal to 4")
    _eq(index.dim(), 3, "index.dim() does not equal to 3")
    B, C, N2, K = grad_output.shape
    _eq(index.size(0), B, "index.size(0) does not equal to batch_size")
    _eq(index.size(1), N2, "index.size(1) does not equal to num_select")
    _eq(index.size(2), K, "index.size(2) does not equal to k")
    N1 = int(num_points)
    idx = index.contiguous()
    return _scatter_backward(
        "group_points_backward", grad_output, idx, None, B, C, N1, N2 * K, K, plan,
        lambda grad_in, *ws: _call(
            _entry("group_points_bwd", grad_output), grad_output, grad_output.data_ptr(), *grad_output.stride(),
            idx.data_ptr(), B, C, N1, N2, K, grad_in.data_ptr(), *ws))


def _plan_buffer(B, num_dest, num_src, device):
    """Device buffer of a sort plan (include/regnet_hip.h: regnet_scatter_plan_bytes), which is also the workspace of the
    float64 backwards (regnet_scatter_f64_workspace_bytes: the same size)."""
    n = _L.regnet_scatter_plan_bytes(B, num_dest, num_src)
    return torch.empty((max(n, 16),), dtype=torch.uint8, device=device)


PLANS = {"built": 0}     # scatter plans built since import (tests, bench)


class ScatterPlan:
    """The sort plan of one destination table (include/regnet_hip.h: regnet_scatter_plan): per scene, the source positions
    of every destination in ascending order.  It depends on the indices alone, so one plan serves every deterministic
    backward of the table (the grouping backward of a pre-multiplied layer's ``dU`` and any other gradient grouped by the
    same neighbours).  ``buffer`` holds it on the device; ``index`` is the table it was built from."""
    __slots__ = ("index", "num_dest", "num_src", "buffer")


def scatter_plan(index, num_dest):
    """index (B, ...) int64 GPU tensor of destinations in [0, num_dest) (others are skipped) -> ScatterPlan, built on the
    current stream.  RuntimeError when the table exceeds the plan kernels' limits."""
    _need_i64(index, "index")
    B = index.size(0)
    idx = index.contiguous()
    L = idx.numel() // max(B, 1)
    R = int(num_dest)
    buf = _plan_buffer(B, R, L, index.device)
    _call("regnet_scatter_plan", index, idx.data_ptr(), B, R, L, buf.data_ptr())
    PLANS["built"] += 1
    p = ScatterPlan()
    p.index, p.num_dest, p.num_src, p.buffer = idx, R, L, buf
    return p


def _scatter_backward(op, go, idx, weight, B, C, R, L, inner, plan, native):
    """The backward of ``op`` -> grad_in (B, C, R): ``go`` (B, C, rows[, inner]) scatter-added by the contiguous index
    ``idx`` (B, L = rows * inner), weighted by ``weight`` (B, L) for interpolate (inner = 3).  ``native(grad_in[, ws])``
    calls the op's own entry point for the dtype of ``go``: float64 with the workspace pointer ``ws``, float32 (the
    atomics kernel) without.  float64, and float32 in deterministic mode, sum each destination in
    ascending source position (csrc/scatter.hip; float32 through ``plan``, ``scatter_plan(idx, R)`` when given, else
    built here).  In deterministic mode a shape with no deterministic kernel goes to determinism.unsupported, which
    raises or (warn_only) lets the default kernel run."""
    grad_in = torch.empty((B, C, R), dtype=go.dtype, device=go.device)
    if go.dtype == torch.float64:
        ws = _plan_buffer(B, R, L, go.device)      # held until the call has enqueued every kernel that uses it
        native(grad_in, ws.data_ptr())
        return grad_in
    if determinism.enabled():
        if plan is not None and (plan.index is not idx or plan.num_dest != R or plan.num_src != L):
            raise RuntimeError("%s: the plan was built for another table" % op)
        try:
            if plan is None:
                plan = scatter_plan(idx, R)
        except RuntimeError:
            determinism.unsupported(op, "%d destinations / %d sources per scene" % (R, L))
        else:
            sb, sc, s_hi, s_lo = (go.stride() + (0,))[:4]
            st = _call("regnet_scatter_segsum_f32", go, go.data_ptr(), sb, sc, s_hi, s_lo, inner,
                       weight.data_ptr() if weight is not None else None, B, C, R, L, plan.buffer.data_ptr(),
                       grad_in.data_ptr(), tolerate=determinism.REGNET_ERR_UNSUPPORTED)
            if st != determinism.REGNET_ERR_UNSUPPORTED:
                return grad_in
            determinism.unsupported(op, "%d channels" % C)
    native(grad_in)
    return grad_in


def point_search(query_xyz, key_xyz, num_neighbours):
    """query (B,3,N1), key (B,3,N2) -> [index (B,N1,3) int64, squared distance (B,N1,3)].
    csrc/interpolate_kernel.cu:88-128."""
    f64 = _need_float(query_xyz, "query_xyz")
    _need_float(key_xyz, "key_xyz", query_xyz)
    B, _, N1 = query_xyz.shape
    N2 = key_xyz.size(2)
    _eq(key_xyz.size(0), B, "key_xyz.size(0) does not equal to batch_size")
    _eq(query_xyz.size(1), 3, "query_xyz.size(1) does not equal to 3")
    _eq(key_xyz.size(1), 3, "key_xyz.size(1) does not equal to 3")
    _eq(int(num_neighbours), 3, "num_neighbours does not equal to K")
    if not N2 >= 3:
        raise RuntimeError("num_key is less than num_neighbours")
    index = torch.empty((B, N1, 3), dtype=torch.int64, device=query_xyz.device)
    dist = torch.empty((B, N1, 3), dtype=query_xyz.dtype, device=query_xyz.device)
    if not f64 and N2 >= GRID_MIN_POINTS and B > 0:
        ws = torch.empty((_L.regnet_grid_workspace_bytes(B, N2),), dtype=torch.uint8, device=query_xyz.device)
        _call("regnet_three_nn_grid_f32", query_xyz, query_xyz.data_ptr(), *query_xyz.stride(), key_xyz.data_ptr(),
              *key_xyz.stride(), B, N1, N2, index.data_ptr(), dist.data_ptr(), ws.data_ptr())
    else:
        _call(_entry("three_nn", query_xyz), query_xyz, query_xyz.data_ptr(), *query_xyz.stride(), key_xyz.data_ptr(),
              *key_xyz.stride(), B, N1, N2, index.data_ptr(), dist.data_ptr())
    return [index, dist]


def _check_interp(first, index, weight, B, N):
    _need_i64(index, "index")
    _need_float(weight, "weight", first)
    _eq(index.dim(), 3, "index.dim() does not equal to 3")
    _eq(weight.dim(), 3, "weight.dim() does not equal to 3")
    _eq(index.size(0), B, "index.size(0) does not equal to batch_size")
    _eq(index.size(1), N, "index.size(1) does not equal to num_select")
    _eq(index.size(2), 3, "index.size(2) does not equal to K")
    _eq(weight.size(0), B, "weight.size(0) does not equal to batch_size")
    _eq(weight.size(1), N, "weight.size(1) does not equal to num_select")
    _eq(weight.size(2), 3, "weight.size(2) does not equal to K")


def interpolate_forward(input, index, weight):
    """input (B,C,M), index/weight (B,N,3) -> (B,C,N).  csrc/interpolate_kernel.cu:187-232."""
    _need_float(input, "input")
    B, C, M = input.shape
    N = index.size(1)
    _check_interp(input, index, weight, B, N)
    idx, w = index.contiguous(), weight.contiguous()
    out = torch.empty((B, C, N), dtype=input.dtype, device=input.device)
    _call(_entry("interpolate_fwd", input), input, input.data_ptr(), *input.stride(), idx.data_ptr(), w.data_ptr(), B, C,
          M, N, out.data_ptr())
    return out


def interpolate_backward(grad_output, index, weight, num_inst):
    """grad_output (B,C,N) -> grad_input (B,C,M).  csrc/interpolate_kernel.cu:292-337.  float64, and float32 in
    deterministic mode: summed in ascending (n, k) order per destination (adding the float32 products g * w), run to run
    bit-identical."""
    _need_float(grad_output, "grad_output")
    B, C, N = grad_output.shape
    _check_interp(grad_output, index, weight, B, N)
    M = int(num_inst)
    idx, w = index.contiguous(), weight.contiguous()
    return _scatter_backward(
        "interpolate_backward", grad_output, idx, w, B, C, M, N * 3, 3, None,
        lambda grad_in, *ws: _call(
            _entry("interpolate_bwd", grad_output), grad_output, grad_output.data_ptr(), *grad_output.stride(),
            idx.data_ptr(), w.data_ptr(), B, C, M, N, grad_in.data_ptr(), *ws))
