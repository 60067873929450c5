"""Per-point (1x1) convolution of the shared-MLP blocks for TRAINING on the GPU, as plain GEMMs in the tensors' own
channel-first layout (nn/modules/conv.py:20-36, :60-76: ``nn.Conv1d/2d(kernel_size=1, bias=False)``).

Why not ``F.conv2d``: MIOpen computes the weight gradient of these layers with an NHWC implicit-GEMM kernel and therefore
transposes the (B,C,L) activation and gradient tensors (up to 1.3 GB each) to channels-last and back on every call --
measured 3.6 ms of ``batched_transpose`` + 5.4 ms of ``igemm_wrw`` per iteration at 4 scenes.  Both operands of
dW[o,i] = sum_{b,l} dY[b,o,l] X[b,i,l] are already K-major in memory, so it is a batched GEMM over chunks of the point
axis (split-K: the output is only C_out x C_in) followed by a small sum; forward and input gradient are one batched GEMM
each.  Same values up to fp32 summation order.
"""
import collections
import threading

import torch

from . import _lib, determinism, fused

ENABLED = True     # module switches (bench.py --set conv1x1_train.ENABLED=0); nothing in the product reads the environment
# 1: forward / input gradient / weight gradient on this repo's own fp32-MFMA kernels (csrc/tgemm.hip) whenever the
# shape qualifies (channel counts multiples of 16, see regnet_conv1x1_train_supported); 0: rocBLAS batched GEMMs only
NATIVE = True
# forward / input gradient by the persistent ticket-driven kernel (csrc/tgemm.hip: tgemm_stream_kernel); 0: one workgroup per tile
STREAM = True
# conv -> bn -> relu -> conv inside a shared-MLP stack without the normalised activation: the first convolution's BatchNorm is
# evaluated as statistics only, the second convolution applies the normalisation + ReLU to its operand fragments (forward and
# weight gradient) and runs the BatchNorm's backward on its input gradient (csrc/tgemm.hip B_AFFINE, bn_train.Pending)
DEFER_BN = True
# input channel counts without a native tile (259, 515, 3: [xyz | feature] rows) are zero-padded to the next multiple of 16
# (at least 32) so that all three contractions stay on csrc/tgemm.hip (Route.pad); 0: rocBLAS batched GEMMs for them
PAD_CHANNELS = True
# EXPERIMENT, off: forward / input gradient with fp32-faithful products on the bf16 matrix pipe (csrc/tsplit.hip: every
# operand as three bf16 pieces, six products, fp32 accumulation).  Never a default path; bench.py reports it under its own name.
SPLIT_PRODUCTS = False
# the statistics pass of the BatchNorm that follows a convolution taken from the convolution's output tiles while they are in
# registers (csrc/tgemm.hip STATS: per-channel sum / sum of squares in fp64), so that bn_train does not read the output for them.
# Not under torch.use_deterministic_algorithms (determinism.py): the kernel adds its partials with fp64 atomics, so bn_train's
# deterministic statistics pass runs instead.
FUSE_STATS = True
DEFERRED = {"layers": 0}     # convolutions that consumed a pending BatchNorm since import (tests, bench)
STATS_FUSED = {"layers": 0}  # convolutions that left the following BatchNorm's statistics since import


def reserve_stream_slots(slots):
    """Leave ``slots`` of the persistent kernels' 2 x CUs workgroup slots empty from now on (csrc/tgemm.hip); returns the
    previous value.  ``train_step`` reserves some while the segmentation head's backward runs beside the region stage."""
    return int(_lib.lib.regnet_conv1x1_stream_reserve_slots(int(slots)))


# The kernels of one layer: ``fwd`` stream | tile | split | smallci | bmm; ``pad``: input channels after zero padding, or 0;
# ``stats``: the forward fills ``sums`` (only where fwd is stream or smallci); ``dgrad`` stream | tile | split | bmm; ``wgrad``
# tgemm | smallci | bmm.
Route = collections.namedtuple("Route", "fwd pad stats dgrad wgrad")


def route(B, Co, Ci, L, *, aligned=True, affine=False, want_stats=False, direct=False):
    """The one place that chooses a layer's kernels, from the module switches, the deterministic mode and the C predicates
    (the only statement of the shape limits); host only, plain integers.  ``aligned``: the input starts on 16 bytes;
    ``affine``: the convolution consumes a bn_train.Pending -- None where it cannot; ``want_stats``: a training BatchNorm
    follows; ``direct``: a native_* wrapper called on its own (tests, bench scripts) -- the shape counts as native, the entry
    point rejects what it does not take.  (``B``: no rule reads it today.)"""
    lib = _lib.lib
    if affine and not direct and not (DEFER_BN and STREAM and NATIVE and lib.regnet_conv1x1_bnrelu_supported(Co, Ci, L)):
        return None
    C = Ci
    native = direct or affine or (NATIVE and bool(lib.regnet_conv1x1_train_supported(Co, Ci, L)))
    if not native and NATIVE and PAD_CHANNELS and Ci > 8 and L % 16 == 0:
        C = max(32, (Ci + 15) // 16 * 16)      # 259 -> 272, 515 -> 528, 9 -> 32: [xyz | feature] rows
        native = C != Ci and bool(lib.regnet_conv1x1_train_supported(Co, C, L))
    fuse = want_stats and FUSE_STATS and not determinism.enabled()
    if native:
        pad, wgrad = (C if C != Ci else 0), ("tgemm" if L % 16 == 0 else "bmm")
        if SPLIT_PRODUCTS and lib.regnet_conv1x1_split_supported(Co, C, L) and (not affine or C <= 1024):
            return Route("split", pad, False, "split", wgrad)
        kind = "stream" if STREAM else "tile"
        stats = bool(fuse and STREAM and lib.regnet_conv1x1_fwd_stats_supported(Co, C, L, int(affine)))
        return Route(kind, pad, stats, kind, wgrad)
    if NATIVE and Ci <= 8 and L % 4 == 0 and aligned:    # a handful of channels: store streams; the input gradient is a tiny GEMM
        return Route("smallci", 0, bool(fuse), "bmm", "smallci")
    return Route("bmm", 0, False, "bmm", "bmm")


# The native_* wrappers below keep tensor-only signatures (bench.py --train brackets them by name, scripts call them on their
# own), so a layer hands them its route here; without one they ask ``route(direct=True)``.
_LAYER = threading.local()


def _routed(r, fn, *args):
    _LAYER.route = r
    try:
        return fn(*args)
    finally:
        _LAYER.route = None


def _route_of_call(B, Co, Ci, L, affine=False):
    return getattr(_LAYER, "route", None) or route(B, Co, Ci, L, affine=affine, direct=True)


def _split(transposed, w, x, B, Co, Ci, L, scale=None, shift=None, relu=0):
    """``regnet_conv1x1_split_f32``: x (B, K, L) -> (B, M, L) with (M, K) = (Co, Ci) forward, (Ci, Co) transposed."""
    out = torch.empty((B, Ci if transposed else Co, L), dtype=torch.float32, device=x.device)
    ws = torch.empty((_lib.lib.regnet_conv1x1_split_workspace_bytes(Co, Ci, transposed),), dtype=torch.uint8, device=x.device)
    _lib.call("regnet_conv1x1_split_f32", x, transposed, w.data_ptr(), x.data_ptr(), out.data_ptr(), B, Co, Ci, L,
              scale.data_ptr() if scale is not None else None, shift.data_ptr() if shift is not None else None, int(relu),
              ws.data_ptr())
    return out


def _pointwise(conv, x):
    """``conv`` is a kernel-size-1, stride-1, ungrouped Conv1d / Conv2d for the non-empty (B, C, ...) input ``x``."""
    one, zero = (1,) * (x.dim() - 2), (0,) * (x.dim() - 2)
    return (tuple(conv.kernel_size) == one and tuple(conv.stride) == one and tuple(conv.dilation) == one
            and tuple(conv.padding) == zero and conv.groups == 1 and x.numel() > 0)


def supported(conv, x):
    return (ENABLED and x.is_cuda and x.dtype == torch.float32 and x.dim() in (3, 4) and conv.bias is None
            and _pointwise(conv, x))


# ---- thin wrappers of the native kernels (module-level names so bench.py --train can bracket them with events) --------
def stats_ok(Co, Ci, L, affine=False):
    """The forward of this shape can leave the statistics of the BatchNorm that follows it (``sums`` of native_fwd /
    native_fwd_bnrelu)."""
    r = route(1, Co, Ci, L, affine=affine, want_stats=True)
    return r is not None and r.stats and r.fwd == "stream" and not r.pad


def new_sums(Co, device):
    STATS_FUSED["layers"] += 1
    return torch.empty((2 * Co,), dtype=torch.float64, device=device)


def native_fwd(x, w, sums=None):
    """x (B, Ci, L) contiguous, w (Co, Ci) contiguous -> Y (B, Co, L) on csrc/tgemm.hip.  ``sums`` (2 Co float64, see
    ``stats_ok``): filled with the per-channel sum and sum of squares of Y."""
    B, Ci, L = x.shape
    Co = w.shape[0]
    kind = "stats" if sums is not None else _route_of_call(B, Co, Ci, L).fwd
    if kind == "split":
        return _split(0, w, x, B, Co, Ci, L)
    y = torch.empty((B, Co, L), dtype=torch.float32, device=x.device)
    if kind == "stats":
        _lib.call("regnet_conv1x1_fwd_stats_stream_f32", x, w.data_ptr(), x.data_ptr(), y.data_ptr(), B, Co, Ci, L, None, None,
                  0, fused._tickets(x.device).data_ptr(), sums.data_ptr())
    elif kind == "stream":
        _lib.call("regnet_conv1x1_fwd_stream_f32", x, w.data_ptr(), x.data_ptr(), y.data_ptr(), B, Co, Ci, L,
                  fused._tickets(x.device).data_ptr())
    else:
        _lib.call("regnet_conv1x1_fwd_f32", x, w.data_ptr(), x.data_ptr(), y.data_ptr(), B, Co, Ci, L)
    return y


def native_dgrad(w, dy):
    """w (Co, Ci), dy (B, Co, L), both contiguous -> dX (B, Ci, L)."""
    B, Co, L = dy.shape
    Ci = w.shape[1]
    kind = _route_of_call(B, Co, Ci, L).dgrad
    if kind == "split":
        return _split(1, w, dy, B, Co, Ci, L)
    dx = torch.empty((B, Ci, L), dtype=torch.float32, device=dy.device)
    if kind == "stream":
            _lib.call("regnet_conv1x1_dgrad_stream_f32", dy, w.data_ptr(), dy.data_ptr(), dx.data_ptr(), B, Co, Ci, L,
                  fused._tickets(dy.device).data_ptr())
    else:
        _lib.call("regnet_conv1x1_dgrad_f32", dy, w.data_ptr(), dy.data_ptr(), dx.data_ptr(), B, Co, Ci, L)
    return dx


def native_wgrad(dy, x):
    """dy (B, Co, L), x (B, Ci, L), both contiguous -> dW (Co, Ci); deterministic split over the point axis."""
    B, Co, L = dy.shape
    Ci = x.shape[1]
    dw = torch.empty((Co, Ci), dtype=torch.float32, device=x.device)
    ws_bytes = _lib.lib.regnet_conv1x1_wgrad_workspace_bytes(B, Co, Ci, L)
    ws = torch.empty((ws_bytes,), dtype=torch.uint8, device=x.device) if ws_bytes else None
    _lib.call("regnet_conv1x1_wgrad_f32", x, dy.data_ptr(), x.data_ptr(), dw.data_ptr(), B, Co, Ci, L,
              ws.data_ptr() if ws is not None else None)
    return dw


def native_fwd_bnrelu(x, w, scale, shift, relu, sums=None):
    """Y = W . [relu](scale * x + shift) (per input channel), x (B, Ci, L) contiguous: the forward of a convolution that
    consumes a pending training BatchNorm (csrc/tgemm.hip: tgemm_stream_kernel<.., B_AFFINE>).  ``sums``: as native_fwd."""
    B, Ci, L = x.shape
    Co = w.shape[0]
    if sums is None and _route_of_call(B, Co, Ci, L, affine=True).fwd == "split":
        return _split(0, w, x, B, Co, Ci, L, scale, shift, relu)
    y = torch.empty((B, Co, L), dtype=torch.float32, device=x.device)
    if sums is not None:
        _lib.call("regnet_conv1x1_fwd_stats_stream_f32", x, w.data_ptr(), x.data_ptr(), y.data_ptr(), B, Co, Ci, L,
                  scale.data_ptr(), shift.data_ptr(), relu, fused._tickets(x.device).data_ptr(), sums.data_ptr())
        return y
    _lib.call("regnet_conv1x1_fwd_bnrelu_stream_f32", x, w.data_ptr(), x.data_ptr(), y.data_ptr(), B, Co, Ci, L,
              scale.data_ptr(), shift.data_ptr(), relu, fused._tickets(x.device).data_ptr())
    return y


def native_wgrad_bnrelu(dy, x, scale, shift, relu):
    """dW = sum_b dY[b] . ([relu](scale * x[b] + shift))^T: the weight gradient of that convolution."""
    B, Co, L = dy.shape
    Ci = x.shape[1]
    dw = torch.empty((Co, Ci), dtype=torch.float32, device=x.device)
    ws_bytes = _lib.lib.regnet_conv1x1_wgrad_workspace_bytes(B, Co, Ci, L)
    ws = torch.empty((ws_bytes,), dtype=torch.uint8, device=x.device) if ws_bytes else None
    _lib.call("regnet_conv1x1_wgrad_bnrelu_f32", x, dy.data_ptr(), x.data_ptr(), dw.data_ptr(), B, Co, Ci, L, scale.data_ptr(),
              shift.data_ptr(), relu, ws.data_ptr() if ws is not None else None)
    return dw


# what bench.py --train brackets: name -> meta(args)
TIMED_OPS = {
    "native_fwd_bnrelu": lambda x, w, scale, shift, relu, sums=None: "B%d Co%d Ci%d L%d flop%d" % (
        x.shape[0], w.shape[0], x.shape[1], x.shape[2], 2 * x.shape[0] * w.shape[0] * x.shape[1] * x.shape[2]),
    "native_wgrad_bnrelu": lambda dy, x, scale, shift, relu: "B%d Co%d Ci%d L%d flop%d" % (
        dy.shape[0], dy.shape[1], x.shape[1], x.shape[2], 2 * dy.shape[0] * dy.shape[1] * x.shape[1] * x.shape[2]),
    "native_fwd": lambda x, w, sums=None: "B%d Co%d Ci%d L%d flop%d" % (x.shape[0], w.shape[0], x.shape[1], x.shape[2],
                                                             2 * x.shape[0] * w.shape[0] * x.shape[1] * x.shape[2]),
    "native_dgrad": lambda w, dy: "B%d Co%d Ci%d L%d flop%d" % (dy.shape[0], w.shape[0], w.shape[1], dy.shape[2],
                                                                2 * dy.shape[0] * w.shape[0] * w.shape[1] * dy.shape[2]),
    "native_wgrad": lambda dy, x: "B%d Co%d Ci%d L%d flop%d" % (dy.shape[0], dy.shape[1], x.shape[1], x.shape[2],
                                                                2 * dy.shape[0] * dy.shape[1] * x.shape[1] * x.shape[2]),
}


def _bmm_wgrad(dy, x):
    """dy (B, Co, L), x (B, Ci, L) -> dW (Co, Ci) by rocBLAS: one batched GEMM per scene over chunks of the point axis (a power
    of two dividing L, enough (chunk x tile) GEMMs for ~1000 workgroups, chunks of at least 1024 points), then a small sum."""
    B, Co, L = dy.shape
    Ci = x.shape[1]
    tiles = ((Co + 127) // 128) * ((Ci + 127) // 128)
    S = 1
    while L % (2 * S) == 0 and L // (2 * S) >= 1024 and S * tiles * B < 1024:
        S *= 2
    Ls = L // S
    part = torch.empty((B, S, Co, Ci), dtype=torch.float32, device=x.device)
    for b in range(B):
        xs = x[b].view(Ci, S, Ls).permute(1, 2, 0)       # (S, Ls, Ci): a strided view, no copy
        ds = dy[b].view(Co, S, Ls).transpose(0, 1)       # (S, Co, Ls)
        torch.bmm(ds, xs, out=part[b])
    return part.sum((0, 1)) if B * S > 1 else part.view(Co, Ci)


def native_fwd_smallci(x, w, sums=None):
    """x (B, Ci <= 8, L) contiguous, w (Co, Ci) contiguous -> Y (B, Co, L): a store stream (csrc/tgemm.hip: conv_smallci_kernel).
    ``sums`` (2 Co float64): filled with the per-channel sum / sum of squares of Y, from the input's moments."""
    B, Ci, L = x.shape
    Co = w.shape[0]
    y = torch.empty((B, Co, L), dtype=torch.float32, device=x.device)
    if sums is not None:
        ws = torch.empty((_lib.lib.regnet_conv1x1_smallci_stats_workspace_bytes(B, Ci, L) // 8,), dtype=torch.float64,
                         device=x.device)
        _lib.call("regnet_conv1x1_fwd_smallci_stats_f32", x, w.data_ptr(), x.data_ptr(), y.data_ptr(), B, Co, Ci, L,
                  ws.data_ptr(), sums.data_ptr())
        return y
    _lib.call("regnet_conv1x1_fwd_smallci_f32", x, w.data_ptr(), x.data_ptr(), y.data_ptr(), B, Co, Ci, L)
    return y


def native_wgrad_smallci(dy, x):
    """dy (B, Co, L), x (B, Ci <= 8, L), both contiguous -> dW (Co, Ci): partial matrices per scene and slice
    (csrc/tgemm.hip: wgrad_smallci_kernel), summed in a fixed order."""
    B, Co, L = dy.shape
    Ci = x.shape[1]
    n = int(_lib.lib.regnet_conv1x1_wgrad_smallci_partials(B, Co, L))
    part = torch.empty((n, Co, Ci), dtype=torch.float32, device=x.device)
    _lib.call("regnet_conv1x1_wgrad_smallci_f32", x, dy.data_ptr(), x.data_ptr(), part.data_ptr(), B, Co, Ci, L)
    return part.sum(0) if n > 1 else part.view(Co, Ci)


class _ConvSmallCo(torch.autograd.Function):
    """y = W . x + bias for 1 <= Co <= 4 output channels (csrc/tgemm.hip: conv_smallco_*): x (B, Ci, L) contiguous, w (Co, Ci),
    bias (Co) or None."""

    @staticmethod
    def forward(ctx, x, w, bias):
        B, Ci, L = x.shape
        Co = w.shape[0]
        w = w.contiguous()
        y = torch.empty((B, Co, L), dtype=torch.float32, device=x.device)
        _lib.call("regnet_conv1x1_smallco_f32", x, 0, w.data_ptr(), bias.data_ptr() if bias is not None else None, x.data_ptr(),
                  y.data_ptr(), B, Co, Ci, L)
        ctx.save_for_backward(x, w)
        ctx.has_bias = bias is not None
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w = ctx.saved_tensors
        dy = dy.contiguous()
        B, Ci, L = x.shape
        Co = w.shape[0]
        dx = dw = db = None
        if ctx.needs_input_grad[0]:
            dx = torch.empty_like(x)
            _lib.call("regnet_conv1x1_smallco_f32", x, 1, w.data_ptr(), None, dy.data_ptr(), dx.data_ptr(), B, Co, Ci, L)
        if ctx.needs_input_grad[1]:
            dw = native_wgrad_smallci(x, dy).t().contiguous()       # (Ci, Co) partial sums with the roles swapped -> (Co, Ci)
        if ctx.has_bias and ctx.needs_input_grad[2]:
            db = dy.sum((0, 2))
        return dx, dw, db


def small_co_ok(conv, x):
    """``conv`` is a kernel-size-1 Conv1d / Conv2d with at most 4 output channels (with or without bias) that the store-stream
    kernels take for the CUDA float32 input ``x``."""
    if not (ENABLED and NATIVE and x.is_cuda and x.dtype == torch.float32 and x.dim() in (3, 4) and conv.weight.shape[0] <= 4
            and _pointwise(conv, x)):
        return False
    L = x.numel() // (x.shape[0] * x.shape[1])
    return L % 4 == 0 and conv.weight.shape[1] <= 4096


def conv1x1_small_co(conv, x):
    """``conv(x)`` for such a layer; check ``small_co_ok`` first."""
    B, Ci = x.shape[0], x.shape[1]
    Co = conv.weight.shape[0]
    xc = x.contiguous().view(B, Ci, -1)
    if xc.data_ptr() % 16:
        xc = xc.clone()
    y = _ConvSmallCo.apply(xc, conv.weight.view(Co, Ci), conv.bias)
    return y.view(B, Co, *x.shape[2:])


class _Conv1x1(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, r, sums=None):
        """x (B, Ci, L) contiguous, w (Co, Ci) -> (B, Co, L) on the kernels of ``r = route(B, Co, Ci, L, ...)``, which the
        backward takes too; ``sums``: see native_fwd, given iff ``r.stats``."""
        B, Ci, L = x.shape
        if r.pad:
            # an input channel count csrc/tgemm.hip has no tile for: zero channels are appended to x and zero columns to w (exact:
            # they add 0.0 to every sum), so that all three contractions run on the native kernels instead of rocBLAS batched
            # GEMMs (8 launches per layer and scene in the backward)
            xp = torch.zeros((B, r.pad, L), dtype=torch.float32, device=x.device)
            xp[:, :Ci].copy_(x)
            wp = torch.zeros((w.shape[0], r.pad), dtype=torch.float32, device=x.device)
            wp[:, :Ci].copy_(w)
            x, w = xp, wp
        ctx.save_for_backward(x, w)
        ctx.route, ctx.Ci = r, Ci
        if r.fwd == "smallci":
            return native_fwd_smallci(x, w.contiguous(), sums)
        if r.fwd == "bmm":
            # bmm on the expanded weight, NOT torch.matmul: for (2-D, 3-D) operands matmul folds the batch by transposing the
            # activation -- a full copy each way
            return torch.bmm(w.unsqueeze(0).expand(B, -1, -1), x)
        return _routed(r, native_fwd, x, w.contiguous(), sums)

    @staticmethod
    def backward(ctx, dy):
        x, w = ctx.saved_tensors
        r = ctx.route
        dy = dy.contiguous()
        dx = dw = None
        if ctx.needs_input_grad[0]:
            if r.dgrad == "bmm":
                dx = torch.bmm(w.t().unsqueeze(0).expand(x.shape[0], -1, -1), dy)
            else:
                dx = _routed(r, native_dgrad, w.contiguous(), dy)
        if ctx.needs_input_grad[1]:
            if r.wgrad == "tgemm":
                dw = native_wgrad(dy, x)
            # dy is the one operand the route could not see: the store-stream kernel reads it in 16-byte pieces
            elif r.wgrad == "smallci" and dy.data_ptr() % 16 == 0:
                dw = native_wgrad_smallci(dy, x)
            else:
                dw = _bmm_wgrad(dy, x)
        if r.pad:
            dx, dw = (None if t is None else t[:, :ctx.Ci] for t in (dx, dw))
        return dx, dw, None, None


class _BnReluConv(torch.autograd.Function):
    """y = W . [relu](bn(x)) with bn in training mode, given bn's statistics (bn_train.Pending): one node for the BatchNorm's
    apply, the ReLU and the convolution; [relu](bn(x)) is never stored.  ``r``: the layer's ``route(..., affine=True)``."""

    @staticmethod
    def forward(ctx, x, gamma, beta, w, mean, invstd, scale, shift, relu, r, sums=None):
        w = w.contiguous()
        y = _routed(r, native_fwd_bnrelu, x, w, scale, shift, relu, sums)
        ctx.save_for_backward(x, gamma, beta, w, mean, invstd, scale, shift)
        ctx.relu, ctx.route = relu, r
        return y

    @staticmethod
    def backward(ctx, dy):
        from . import bn_train
        x, gamma, beta, w, mean, invstd, scale, shift = ctx.saved_tensors
        dy = dy.contiguous()
        dz = _routed(ctx.route, native_dgrad, w, dy)
        dw = native_wgrad_bnrelu(dy, x, scale, shift, ctx.relu) if ctx.needs_input_grad[3] else None
        dx, dgamma, dbeta = bn_train.bn_backward(x, dz, gamma, beta, mean, invstd, ctx.relu)
        return dx, dgamma, dbeta, dw, None, None, None, None, None, None, None


def pending_ok(conv, x):
    """``conv`` can consume a bn_train.Pending whose BatchNorm input is ``x`` (shape of the activation)."""
    if not supported(conv, x):
        return False
    B, Ci = x.shape[0], x.shape[1]
    return route(B, conv.weight.shape[0], Ci, x.numel() // (B * Ci), affine=True) is not None


def _with_sums(y, sums):
    """Hands the statistics a convolution left (``sums``) to the BatchNorm that consumes its output: an attribute of the very
    tensor object the block passes on (bn_train.bn_stats / bn_relu look for it)."""
    if sums is not None:
        y._bn_sums = sums
    return y


def conv1x1_of_pending(conv, pending, shape, stats=False):
    """``conv([relu](bn(x)))`` for a bn_train.Pending of that BatchNorm; ``shape``: of x as the stack sees it ((B,C,N) or
    (B,C,N,K)); check ``pending_ok`` first.  ``stats``: a training BatchNorm follows -- leave its statistics with the output."""
    B, Ci = shape[0], shape[1]
    Co = conv.weight.shape[0]
    DEFERRED["layers"] += 1
    x = pending.x.view(B, Ci, -1)
    r = route(B, Co, Ci, x.shape[2], affine=True, want_stats=stats)
    sums = new_sums(Co, x.device) if r.stats else None
    y = _BnReluConv.apply(x, pending.gamma, pending.beta, conv.weight.view(Co, Ci), pending.mean,
                          pending.invstd, pending.scale, pending.shift, pending.relu, r, sums)
    return _with_sums(y.view(B, Co, *shape[2:]), sums)


def gemm_conv(x, w):
    """x (B, Ci, L) contiguous, w (Co, Ci) -> (B, Co, L): the autograd GEMM convolution itself, on the kernels ``route`` gives
    the shape (native, zero-padded, store stream or rocBLAS); it leaves no statistics -- ``conv1x1(stats=True)`` does."""
    B, Ci, L = x.shape
    return _Conv1x1.apply(x, w, route(B, w.shape[0], Ci, L, aligned=x.data_ptr() % 16 == 0))


def conv1x1(conv, x, stats=False):
    """``conv(x)`` for a bias-free kernel-size-1 Conv1d / Conv2d; check ``supported`` first.  ``stats``: a training BatchNorm
    follows -- leave its statistics with the output where the route's forward can (``sums`` is allocated iff ``Route.stats``)."""
    B, Ci = x.shape[0], x.shape[1]
    Co = conv.weight.shape[0]
    xf = x.contiguous().view(B, Ci, -1)
    r = route(B, Co, Ci, xf.shape[2], aligned=xf.data_ptr() % 16 == 0, want_stats=stats)
    sums = new_sums(Co, x.device) if r.stats else None
    y = _Conv1x1.apply(xf, conv.weight.view(Co, Ci), r, sums)
    return _with_sums(y.view(B, Co, *x.shape[2:]), sums)
