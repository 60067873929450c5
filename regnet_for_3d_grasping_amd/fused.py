"""Fused eval-mode forward of the set-abstraction / feature-propagation / head blocks on MI355X.

``pn2_utils.modules`` and ``pointnet2`` dispatch here when ``usable()`` holds (module in eval
mode, autograd off, GPU tensors).  The module API is unchanged -- channel-first ``(B,C,N)``
tensors in and out -- but internally activations are channels-last buffers driven through the
fp32-MFMA shared-MLP kernels of csrc/mlp.hip, and the tensors handed back are transposed *views*
of those buffers (so the next fused block reads them without a copy).

Per block (reference pn2_utils/modules.py:210-246 and :500-509, pointnet2.py:116-119) ``sa_route`` / ``fp_route`` choose one of
these ([...]: one kernel), and the geometry stage, the feature stage and ``prepack`` all follow that choice:
  SA  chain3         FPS -> ball query + pairing -> [gather(feat | xyz - centre) . W1 . W2 . W3 + max over K]
      layer12        FPS -> ball query -> [gather . W1 . W2 (+ max)] (-> [. W3 + max])
      premul_chain*  ... + V = W1x . centre -> U = W1 . [feat | xyz] per SOURCE point -> [relu(U[nbr] - V) . W2 . W3 + max]
      premul_layer   ... -> [relu(U[nbr] - V) . W2 (+ max)] (-> [. W3 + max])
      layer1         FPS -> ball query -> [gather . W1] -> [. W2 (+ max)] (-> [. W3 + max])
  FP  premul         3-NN -> Ys = W1s . sparse (, Yd = W1d . skip) -> [interpolate(Ys) + Yd, BN, ReLU] -> [. W2] (-> [. W3])
      concat         3-NN -> interpolate+concat (channels-last) -> [. W1] -> [. W2] (-> [. W3])
      head_chain     last block: as premul -> [. W2 . W3 . head] -- head_interp: the interpolation in that kernel's prologue
  head: [. W]*4 -> conv_score + bn_score + sigmoid (behind a last block that took neither head route)
Eval-mode BatchNorm is folded into a per-channel (scale, shift) applied in the GEMM epilogue.
"""
import collections
import ctypes

import torch

from . import _lib, pn2_ext

ENABLED = True
CHAIN3 = True   # level-1 set-abstraction block as one register-chained kernel (sa_route: chain3)
SPLITK_MAX_ROWS = 1024   # at most this many rows: the GEMM is "skinny" and is split along K (see mlp_layer)
PREMUL = True   # evaluate the first layer of wide set-abstraction blocks per source point (sa_route: premul_*; fp_route likewise)
PREMUL_CENTRE = True   # ... on mean-centred coordinates (a module switch like the others: bench.py --set fused.PREMUL_CENTRE=0)
ROWCHAIN = True   # last FP block's layers 2-3 + the whole head in one register-chained kernel; level-2 SA block's layers 2-3 + pooling
SA3_CHAIN = True  # level-3 set-abstraction block's layers 2-3 + pooling in one register-chained kernel
FP_HEAD_INTERP = True   # ROWCHAIN's head kernel with the block's first layer (interpolation of the pre-multiplied sparse rows) in its prologue

# The kernels of one set-abstraction block: ``features`` chain3 | layer12 | premul_chain512 | premul_chain256 | premul_layer |
# layer1; ``tail``: plain layers (mlp_layer) behind that kernel, the last of them pooling -- 0: the kernel pools itself;
# ``prepare``: what the geometry stage computes for it: pairs (count, order) | premul (mu, V, V_layer) | None.
SaRoute = collections.namedtuple("SaRoute", "features tail prepare")


def sa_route(module, has_feature=True):
    """The one place that chooses a set-abstraction block's kernels, from the module's shapes and flags and the module
    switches (the only statement of the shape limits); host only: no packed layer, no tensor.  ``has_feature``: the block is
    given point features (the geometry stage sees coordinates only and assumes so).  None: a block the fused forward does not
    cover (supports_sa).  ``prepare`` is premul for the eval-mode forward only: that term is a function of the weights."""
    mlp, n = module.mlp, len(module.mlp)
    if getattr(module.grouper, "num_neighbours", 0) != 64 or n < 2 or (has_feature and not module.use_xyz):
        return None
    width = [block.conv.out_channels for block in mlp]
    relu = [block.relu is not None for block in mlp]
    if mlp[0].conv.in_channels <= 8 and width[0] % 16 == 0 and relu[0]:
        # narrow gathered input (level 1: rgb + xyz): layer 1 is recomputed on the VALU inside layer 2's operand load, its
        # (P x C1) activation never exists in HBM -- or the whole block in one kernel, activations in registers (csrc/sa_chain.hip)
        if CHAIN3 and n == 3 and width[0] == 128 and width[1] == 128 and relu[1] and width[2] % 32 == 0:
            return SaRoute("chain3", 0, "pairs")
        return SaRoute("layer12", n - 2, None)
    if PREMUL and has_feature and relu[0] and width[0] % 4 == 0:
        # wide gathered input (levels 2+; a narrow one of another first width too): layer 1 is linear in [f_j | x_j - x_c], so
        # it is evaluated once per source point and once per centre (N + M rows instead of M * 64) and the gather, the subtraction
        # and the ReLU happen inside layer 2's operand load -- or layers 2 and 3 + the pooling in one kernel (csrc/rowchain.hip)
        prepare = None if module.training or torch.is_grad_enabled() else "premul"
        if SA3_CHAIN and n == 3 and width == [512, 512, 1024] and relu[1]:
            return SaRoute("premul_chain512", 0, prepare)
        if ROWCHAIN and n == 3 and width == [256, 256, 512] and relu[1]:
            return SaRoute("premul_chain256", 0, prepare)
        return SaRoute("premul_layer", n - 2, prepare)
    return SaRoute("layer1", n - 1, None)


# The kernels of one feature-propagation block: ``features`` head_interp | head_chain (the last block and the segmentation
# head as one kernel) | premul | concat; ``skip``: how the dense skip input enters a pre-multiplied first layer: table (at
# most 4 channels: multiplied inside the interpolation) | gemm (a product of its own) | None (no skip input, or concat).
FpRoute = collections.namedtuple("FpRoute", "features skip")


def fp_route(module, Cs, Cd, Ns=None, Nd=None, *, seg=None, f32=True):
    """The one place that chooses a feature-propagation block's kernels; host only, plain integers.  ``Cs`` / ``Cd``:
    channels of the sparse and the dense (skip) input, ``Ns`` / ``Nd``: their points -- None: assume Ns < Nd (prepack knows
    widths only); ``f32``: the skip input is float32.  ``seg``: the PointNet2Seg whose LAST block this is, when the caller
    wants the block and the head as one kernel -- None where that does not apply (the caller runs the two separately)."""
    first = module.mlp[0].conv
    C1 = first.out_channels
    # layer 1 is linear in [interpolated | skip]: multiply the SPARSE rows (and the skip rows by their own weight columns),
    # interpolate the products.  (C1 / 4 lanes walk a row of the interpolation, a block holds a whole number of rows.)
    premul = (PREMUL and f32 and C1 % 4 == 0 and 256 % (C1 // 4) == 0 and Cs % 4 == 0 and Cd >= 0 and (Cd % 4 == 0 or Cd <= 4)
              and (Ns is None or Ns < Nd) and first.in_channels == Cs + Cd)
    skip = None if not premul or Cd == 0 else "table" if Cd <= 4 else "gemm"
    if seg is not None:
        if not (premul and supports_rowchain(seg, module)):
            return None
        return FpRoute("head_interp" if FP_HEAD_INTERP and Cd <= 4 else "head_chain", skip)
    return FpRoute("premul" if premul else "concat", skip)


_call = _lib.call
_L = _lib.lib


def _f32_weights(module):
    p = next(module.parameters(), None)
    return p is None or p.dtype == torch.float32


def usable(module, xyz):
    """The fused chains are float32 kernels: float64 tensors or weights take the operator-granular path."""
    return (ENABLED and xyz.is_cuda and xyz.dtype == torch.float32 and not module.training and not torch.is_grad_enabled()
            and _f32_weights(module))


def supports_sa(module, feature):
    """True when the fused set-abstraction chain covers this module's configuration; otherwise the caller takes the
    operator-granular GPU path (pn2_ext group / torch conv), exactly like the reference."""
    grouper = getattr(module, "grouper", None)
    return (grouper is not None and grouper.num_neighbours == 64 and len(module.mlp) >= 2 and _f32_weights(module)
            and (feature is None or (module.use_xyz and feature.dtype == torch.float32)))


def supports_fp(module, sparse_feature):
    return (sparse_feature.dtype == torch.float32 and _f32_weights(module)
            and getattr(module.interpolator, "num_neighbors", 0) == 3)


def _round_up(x, m):
    return (x + m - 1) // m * m


_ticket_pools = {}


def _tickets(device, n=1):
    """``n`` zeroed int32 work-queue heads for a ticket-driven chain kernel.  Carved out of a pool that is zeroed once per 256
    words ON THE STREAM THAT USES IT (a word is handed out once and never reused): one fill kernel per ~60 feature stages
    instead of one -- and its ~10 us launch gap -- in front of every chain launch."""
    if torch.cuda.is_current_stream_capturing():
        # inside a hipGraph capture (pipeline.StageGraphs): the word is reused by every replay, so its zero-fill is a node of
        # the graph (memory from the graph's private pool)
        return torch.zeros((n,), dtype=torch.int32, device=device)
    stream = torch.cuda.current_stream(device)
    key = (device.index if device.index is not None else torch.cuda.current_device(), stream.cuda_stream)
    pool = _ticket_pools.get(key)
    if pool is None or pool[1] + n > pool[0].numel():
        pool = [torch.zeros((256,), dtype=torch.int32, device=device), 0]
        _ticket_pools[key] = pool
    out = pool[0][pool[1]:pool[1] + n]
    pool[1] += n
    return out


class _Layer:
    """One conv(1x1, bias-free or biased) + eval BatchNorm (+ReLU) packed for the GEMM kernel.  ``derived``: packs computed
    from this one (see ``_derived``), which therefore go away with it."""

    __slots__ = ("W", "W8", "scale", "shift", "N", "K", "Kpad", "relu", "derived")

    def __init__(self, **fields):
        self.W8 = None
        self.derived = {}
        for name, value in fields.items():
            setattr(self, name, value)


def _pack(conv, bn, relu, col_order=None):
    w = conv.weight.detach().reshape(conv.weight.shape[0], -1).float()  # (N, K)
    N, K = w.shape
    if col_order is not None:
        w = w[:, col_order]
        K = w.shape[1]
    L = _Layer(N=N, K=K, Kpad=_round_up(max(K, 1), 16), relu=1 if relu else 0)
    Wp = torch.zeros((_round_up(N, 128), L.Kpad), dtype=torch.float32, device=w.device)
    Wp[:N, :K] = w
    if bn is not None:
        scale = bn.weight.detach().float() / torch.sqrt(bn.running_var.detach().float() + bn.eps)
        shift = bn.bias.detach().float() - bn.running_mean.detach().float() * scale
    else:
        scale = torch.ones(N, dtype=torch.float32, device=w.device)
        shift = torch.zeros(N, dtype=torch.float32, device=w.device)
    if conv.bias is not None:
        shift = shift + conv.bias.detach().float() * scale
    L.W, L.scale, L.shift = Wp.contiguous(), scale.contiguous(), shift.contiguous()
    if K <= 8:  # narrow first layer: also keep the [N][8] form consumed by the layer-1-fused gather kernel
        W8 = torch.zeros((N, 8), dtype=torch.float32, device=w.device)
        W8[:, :K] = w
        L.W8 = W8.contiguous()
    return L


def _signature(module):
    """(address, version) of every parameter and buffer: changes with any in-place update (optimizer step, load_state_dict,
    .to()).  The LIST of tensors is cached on the module -- walking ``parameters()`` / ``buffers()`` is ~15 us per call and a
    forward asks ~30 times -- and re-read by ``prepack`` (every ``ForwardPipeline.run``) or ``forget``: replacing a Parameter
    OBJECT or a sub-module of a network that has already run needs one of the two."""
    tensors = module.__dict__.get("_regnet_sig_tensors")
    if tensors is None:
        tensors = list(module.parameters()) + list(module.buffers())
        module.__dict__["_regnet_sig_tensors"] = tensors
    return tuple((t.data_ptr(), t._version) for t in tensors)


def forget(*nets):
    """Drop the cached tensor lists of ``_signature`` below these networks (after structural surgery on a network)."""
    for net in nets:
        if net is not None:
            for m in net.modules():
                m.__dict__.pop("_regnet_sig_tensors", None)


def _cached(owner, slot, sig, build):
    """The pack ``slot`` of module ``owner``: ``build()``'s value, rebuilt whenever ``sig`` (a ``_signature`` of the modules
    whose weights it is made of) differs from the one it was built with.  Every pack of a module lives in one dict,
    ``owner._regnet_packs``: slot -> (sig, value)."""
    packs = owner.__dict__.setdefault("_regnet_packs", {})
    entry = packs.get(slot)
    if entry is None or entry[0] != sig:
        entry = packs[slot] = (sig, build())
    return entry[1]


def _derived(layer, key, build):
    """A pack computed from the packed layer ``layer`` (and from nothing but its stack pack), kept on it: it lives exactly as
    long as that layer pack."""
    if key not in layer.derived:
        layer.derived[key] = build()
    return layer.derived[key]


def _packed_stack(owner, stack, first_col_order=None):
    """Packed layers of a SharedMLP (list of conv/bn/relu blocks), cached on ``owner`` and rebuilt
    whenever a parameter or BN buffer is modified (in-place updates bump ``_version``).
    ``first_col_order``: optional callable returning the column permutation of the first layer (only
    evaluated on a cache miss -- it involves a host->device copy, which would stall the stream)."""
    def build():
        order = first_col_order() if first_col_order is not None else None
        return [_pack(block.conv, block.bn, block.relu is not None, order if i == 0 else None) for i, block in enumerate(stack)]
    return _cached(owner, "stack", _signature(stack), build)


# ---- thin kernel wrappers (module-level names so bench.py can bracket them with events) ------
def mlp_layer(A, Ka, layer, P, pool_group=0):
    """A: channels-last (P, lda) float32 buffer whose first Ka columns are valid."""
    rows = P // pool_group if pool_group else P
    out = torch.empty((rows, layer.N), dtype=torch.float32, device=A.device)
    if not pool_group and P <= SPLITK_MAX_ROWS and layer.Kpad >= 128:
        # skinny problem (the region heads: B*64 rows): a 128-row tile grid cannot fill the chip, so cut K into
        # slices of >= 64 that run on different workgroups (deterministic: added in order by a second kernel)
        tiles = ((P + 127) // 128) * ((layer.N + 127) // 128)
        ksplit = max(1, min(layer.Kpad // 64, 256 // max(tiles, 1)))
        if ksplit > 1:
            ws = torch.empty((_L.regnet_mlp_splitk_workspace_bytes(P, layer.N, ksplit),), dtype=torch.uint8,
                             device=A.device)
            _call("regnet_mlp_layer_splitk_f32", A, A.data_ptr(), A.stride(0), Ka, layer.W.data_ptr(), layer.Kpad,
                  layer.scale.data_ptr(), layer.shift.data_ptr(), out.data_ptr(), out.stride(0), P, layer.N, layer.relu,
                  ksplit, ws.data_ptr())
            return out
    _call("regnet_mlp_layer_f32", A, A.data_ptr(), A.stride(0), Ka, layer.W.data_ptr(), layer.Kpad, layer.scale.data_ptr(),
          layer.shift.data_ptr(), out.data_ptr(), out.stride(0), P, layer.N, layer.relu, pool_group)
    return out


def _strided3(t):
    """(pointer, batch stride, channel stride, point stride, channels) of a (B,C,N) tensor of any strides; zeros for None."""
    return (None, 0, 0, 0, 0) if t is None else (t.data_ptr(),) + tuple(t.stride()) + (t.size(1),)


def sa_layer1(feature, xyz, nbr, ctr, layer, B, M, group):
    """Gather-fused first SA layer.  feature (B,Cf,N) any strides or None; xyz (B,3,N) any strides."""
    out = torch.empty((B * M * group, layer.N), dtype=torch.float32, device=xyz.device)
    fptr, fb, fc, fn, Cf = _strided3(feature)
    _call("regnet_sa_layer1_f32", xyz, fptr, fb, fn, fc, Cf, xyz.data_ptr(), *xyz.stride(), nbr.data_ptr(), ctr.data_ptr(),
          B, M, group, layer.W.data_ptr(), layer.Kpad, layer.scale.data_ptr(), layer.shift.data_ptr(), out.data_ptr(),
          out.stride(0), layer.N, layer.relu)
    return out


def sa_layer12(feature, xyz, nbr, ctr, first, layer, B, M, group, pool_group=0):
    """Gather + layer 1 (VALU, inside the operand load) + layer 2 (MFMA) of a narrow-input SA block."""
    P = B * M * group
    rows = P // pool_group if pool_group else P
    out = torch.empty((rows, layer.N), dtype=torch.float32, device=xyz.device)
    fptr, fb, fc, fn, Cf = _strided3(feature)
    _call("regnet_sa_layer12_f32", xyz, fptr, fb, fn, fc, Cf, xyz.data_ptr(), *xyz.stride(), nbr.data_ptr(),
          ctr.data_ptr(), B, M, group, first.W8.data_ptr(), first.scale.data_ptr(), first.shift.data_ptr(), first.N,
          layer.W.data_ptr(), layer.Kpad, layer.scale.data_ptr(), layer.shift.data_ptr(), out.data_ptr(), out.stride(0),
          layer.N, layer.relu, pool_group)
    return out


def _premul_layers(first, Cf):
    """Derived packings of a set-abstraction block's first layer (columns [feature | xyz]) for the
    per-source-point evaluation: ``u`` = scale * W [f | x] (no shift, no ReLU) and ``v`` = scale * Wx x_c - shift."""
    def build():
        u = _Layer(W=first.W, scale=first.scale, shift=torch.zeros_like(first.shift), N=first.N, K=first.K, Kpad=first.Kpad,
                   relu=0)
        Wx = torch.zeros((first.W.shape[0], 16), dtype=torch.float32, device=first.W.device)
        Wx[:, :3] = first.W[:, Cf:Cf + 3]
        v = _Layer(W=Wx.contiguous(), scale=first.scale, shift=(-first.shift).contiguous(), N=first.N, K=3, Kpad=16, relu=0)
        return u, v
    return _derived(first, "premul", build)


def _sa_packs(module, route, Cf, device):
    """The packs ``route``'s kernels read (beside a chain's own weight stream, _packed_premul_chain): -> (layers, (u, v) of
    _premul_layers or None).  The reference's channel order is [xyz(3) | feature] (modules.py:52); the kernels gather
    [feature | xyz], so the first layer's weight columns are permuted accordingly."""
    layers = _packed_stack(module, module.mlp, lambda: torch.cat([torch.arange(3, 3 + Cf), torch.arange(0, 3)]).to(device))
    return layers, _premul_layers(layers[0], Cf) if route.features.startswith("premul") else None


def _premul_centres(xyz, new_xyz, v_layer, known=()):
    """What sa_route's ``prepare`` premul stands for: the scene mean ``mu`` (``known``: a plan that may hold it already) and
    the per-centre term ``V`` = W_xyz . (centre - mu) with the first layer's BatchNorm folded in.  U[j] - V[c] = s W [f_j |
    x_j - x_c] - t only up to fp32 rounding of the two big terms: both sides use the coordinates RELATIVE TO THE SCENE'S MEAN
    (the difference is unchanged, the magnitudes -- table-top scenes sit ~0.75 m from the origin -- and with them the
    cancellation error shrink; pack_rows subtracts).  V is a function of the WEIGHTS too, unlike the rest of a plan, so the
    plan keeps the pack it was made with (``V_layer``) and sa_features recomputes V when the block's pack is another by then."""
    mu = known["mu"] if "mu" in known else xyz.mean(dim=2, keepdim=True) if PREMUL_CENTRE else None
    rows = new_xyz.shape[0] * new_xyz.shape[2]
    return {"mu": mu, "V": mlp_layer(pack_rows(None, new_xyz, 4, mu), 4, v_layer, rows), "V_layer": v_layer}


def pack_rows(feature, xyz, width, mu=None):
    """Channels-last rows [feature | xyz - mu | 0] of every point: feature (B,Cf,N) or None, xyz (B,3,N), mu (B,3,1) or None
    -> (B*N, width)."""
    B, _, N = xyz.shape
    out = torch.empty((B * N, width), dtype=torch.float32, device=xyz.device)
    fptr, fb, fc, fn, Cf = _strided3(feature)
    if mu is not None:
        mu = mu.reshape(B, 3)
        mu = mu if mu.is_contiguous() else mu.contiguous()
    _call("regnet_pack_rows_centred_f32", xyz, fptr, fb, fc, fn, Cf, xyz.data_ptr(), *xyz.stride(),
          None if mu is None else mu.data_ptr(), B, N, width, out.data_ptr())
    return out


def sa_premul_layer(U, V, nbr, layer, B, Nsrc, M, group, pool_group=0):
    """Layer 2 of a set-abstraction block over pre-multiplied layer-1 rows: relu(U[nbr] - V[centre]) . W."""
    P = B * M * group
    rows = P // pool_group if pool_group else P
    out = torch.empty((rows, layer.N), dtype=torch.float32, device=U.device)
    _call("regnet_sa_premul_layer_f32", U, U.data_ptr(), U.stride(0), V.data_ptr(), V.stride(0), U.size(1),
          nbr.data_ptr(), B, Nsrc, M, group, layer.W.data_ptr(), layer.Kpad, layer.scale.data_ptr(),
          layer.shift.data_ptr(), out.data_ptr(), out.stride(0), layer.N, layer.relu, pool_group)
    return out


def chain3_order(count):
    """Processing order of sa_chain3's neighbourhoods by cost class (<= 32 members, 33..48, more), stable within a class.
    (The expensive class first instead: 994-1 005 against 995-1 000 scenes/s over three alternations -- no difference.)"""
    c = count.reshape(-1)
    if c.is_cuda and c.dtype == torch.int64 and c.numel() <= (1 << 24):
        return pn2_ext.class_order(c)       # a three-bin counting sort in one launch (six tensor ops + a radix sort before)
    return torch.argsort((c > 32).to(torch.uint8) + (c > 48).to(torch.uint8), stable=True)


def chain3_pair_cost(c_a, c_b):
    """Point tiles that sa_chain3 executes for two neighbourhoods at waves w and w + 4 (int64 tensors of member counts):
    their full tiles plus one shared tile when the two remainders fit 32 rows together, else one tile each."""
    a, b = c_a.clamp(1, 64) - 1, c_b.clamp(1, 64) - 1
    return (a >> 5) + (b >> 5) + 1 + ((a & 31) + (b & 31) + 2 > 32).to(a.dtype)


def _pair_order_host(count):
    """The plan of regnet_pair_order_i64 (csrc/gather.hip: pair_order_kernel) restated in numpy, run for run."""
    import numpy as np
    c = np.clip(np.asarray(count, dtype=np.int64).reshape(-1), 1, 64) - 1
    n = c.size
    bins = ((c & 31) << 1) | (c >> 5)                       # ascending remainder, then full tiles
    work = np.argsort(bins, kind="stable")
    tot = np.bincount(bins, minlength=64)
    base = np.concatenate([[0], np.cumsum(tot)[:-1]])
    runs, carry = [], None                                  # (bin A, start A, bin B, start B, pairs, cost)

    def alone(b, start, left):
        nonlocal carry
        if carry is not None and left > 0:
            runs.append((carry[0], carry[1], b, start, 1, (carry[0] & 1) + 1 + (b & 1) + 1))
            start, left, carry = start + 1, left - 1, None
        q = left >> 1
        if q:
            runs.append((b, start, b, start + q, q, 2 * ((b & 1) + 1)))
        if left & 1:
            carry = (b, start + 2 * q)

    a, z, fa, kz = 0, 63, 0, 0
    while True:
        while a < z and tot[a] - fa == 0:
            a, fa = a + 1, 0
        while z > a and tot[z] - kz == 0:
            z, kz = z - 1, 0
        if a == z:
            avail = tot[a] - fa - kz
            if avail >= 2 and 2 * ((a >> 1) + 1) <= 32:
                q = avail >> 1
                runs.append((a, fa, a, fa + q, q, 2 * (a & 1) + 1))
                fa, avail = fa + 2 * q, avail - 2 * q
            if avail > 0:
                alone(a, fa, avail)
            break
        ra, rz = tot[a] - fa, tot[z] - kz
        if (a >> 1) + 1 + (z >> 1) + 1 <= 32:
            q = min(ra, rz)
            runs.append((a, fa, z, rz - q, q, (a & 1) + (z & 1) + 1))
            fa, kz = fa + q, kz + q
        else:
            alone(z, 0, rz)
            kz += rz
    order = np.empty(n, dtype=np.int64)
    full = (n >> 3) << 2
    nxt = np.concatenate([[0], np.cumsum([sum(r[4] for r in runs if r[5] == k) for k in (1, 2, 3)])])
    for ba, sa, bb, sb, q, cost in runs:
        pp = nxt[cost - 1] + np.arange(q)
        nxt[cost - 1] += q
        host, guest = work[base[ba] + sa + np.arange(q)], work[base[bb] + sb + np.arange(q)]
        slot = np.where(pp < full, 8 * (pp >> 2) + (pp & 3), 2 * full + 2 * (pp - full))
        order[slot] = host
        order[slot + np.where(pp < full, 4, 1)] = guest
    if carry is not None:
        order[n - 1] = work[base[carry[0]] + carry[1]]
    return order


def chain3_pair_order(count):
    """Processing order of sa_chain3's neighbourhoods for its row packing: slots 8 g + w and 8 g + w + 4 (waves w and
    w + 4 of a workgroup) hold two neighbourhoods whose remainders ``(count - 1) % 32 + 1`` share one point tile where the
    greedy matching found a partner, and the pairs are sorted by cost in tiles (``chain3_pair_cost``), light ones first,
    so that whole workgroups are of one cost.  A permutation; which one is sa_chain3's speed only, never its result."""
    c = count.reshape(-1)
    if c.is_cuda and c.dtype == torch.int64 and c.numel() <= (1 << 24):
        return pn2_ext.pair_order(c)
    return torch.from_numpy(_pair_order_host(c.cpu().numpy())).to(c.device)


# EXPERIMENT, off: the level-1 block with fp32-faithful products on the bf16 matrix pipe (csrc/sa_split.hip).  Never a
# default path; bench.py reports it under its own name (value_split_products).
SPLIT_PRODUCTS = False


def sa_chain3_split(feature, xyz, nbr, ctr, l1, l2, l3, B, M, group, count=None, order=None):
    """``sa_chain3`` by ``regnet_sa_chain3_split_f32``; the weights' bf16 pieces are built by the kernel's first launch on
    a layer pack (both layers are of the same stack pack: the planes are kept on ``l3``)."""
    out = torch.empty((B * M, l3.N), dtype=torch.float32, device=xyz.device)
    fptr, fb, fc, fn, Cf = _strided3(feature)
    planes = l3.derived.get("split_planes")
    build = planes is None
    if build:
        planes = l3.derived["split_planes"] = torch.empty((_L.regnet_sa_chain3_split_plane_bytes(l3.N),), dtype=torch.uint8,
                                                          device=xyz.device)
    _call("regnet_sa_chain3_split_f32", xyz, fptr, fb, fn, fc, Cf, xyz.data_ptr(), *xyz.stride(), nbr.data_ptr(), ctr.data_ptr(),
          None if count is None else count.data_ptr(), None if order is None else order.data_ptr(), B, M, group,
          l1.W8.data_ptr(), l1.scale.data_ptr(), l1.shift.data_ptr(), l2.W.data_ptr(), l2.Kpad, l2.scale.data_ptr(),
          l2.shift.data_ptr(), l3.W.data_ptr(), l3.Kpad, l3.scale.data_ptr(), l3.shift.data_ptr(), l3.N, l3.relu,
          planes.data_ptr(), int(build), out.data_ptr(), out.stride(0), _tickets(xyz.device).data_ptr())
    return out


def sa_chain3(feature, xyz, nbr, ctr, l1, l2, l3, B, M, group, count=None, order=None):
    """Whole narrow-input SA block (gather, three layers, max over the neighbours) in one kernel; -> (B*M, C3).
    ``count`` (B,M) int64: members per neighbourhood (half the work for those with <= 32); ``order`` (B*M,) int64:
    processing order of the neighbourhoods (small ones together)."""
    if (SPLIT_PRODUCTS and group == 64 and l2.Kpad == 128 and l3.Kpad == 128 and l3.N == 256 and feature is not None
            and feature.size(1) == 3):      # (the shapes of the level-1 block, the only ones the experiment's kernel is built for)
        return sa_chain3_split(feature, xyz, nbr, ctr, l1, l2, l3, B, M, group, count, order)
    out = torch.empty((B * M, l3.N), dtype=torch.float32, device=xyz.device)
    fptr, fb, fc, fn, Cf = _strided3(feature)
    _call("regnet_sa_chain3_f32", xyz, fptr, fb, fn, fc, Cf, xyz.data_ptr(), *xyz.stride(), nbr.data_ptr(), ctr.data_ptr(),
          None if count is None else count.data_ptr(), None if order is None else order.data_ptr(), B, M, group,
          l1.W8.data_ptr(), l1.scale.data_ptr(), l1.shift.data_ptr(), l1.N,
          l2.W.data_ptr(), l2.Kpad, l2.scale.data_ptr(), l2.shift.data_ptr(), l2.N,
          l3.W.data_ptr(), l3.Kpad, l3.scale.data_ptr(), l3.shift.data_ptr(), l3.N, l3.relu, out.data_ptr(), out.stride(0))
    return out


def interp_concat(sparse_cl, idx, dist2, eps, dense_feature, B, Nd):
    """sparse_cl: (B,Ns,Cs) channels-last contiguous; dense_feature (B,Cd,Nd) any strides or None.
    Returns the (B*Nd, round_up(Cs+Cd,4)) channels-last operand of the first FP layer and its valid width."""
    Cs = sparse_cl.size(2)
    Cd = 0 if dense_feature is None else dense_feature.size(1)
    width = _round_up(Cs + Cd, 4)
    out = torch.empty((B * Nd, width), dtype=torch.float32, device=sparse_cl.device)
    dptr, db, dc, dn, _ = _strided3(dense_feature)
    _call("regnet_interp_concat_f32", sparse_cl, sparse_cl.data_ptr(), sparse_cl.stride(0), sparse_cl.stride(1), Cs,
          idx.data_ptr(), dist2.data_ptr(), float(eps), dptr, db, dn, dc, Cd, B, Nd, out.data_ptr(), out.stride(0), width)
    return out, width


def _fp_split_layers(first, Cs):
    """Derived packings of a feature-propagation block's first layer (columns [interpolated | skip]):
    ``s`` = W[:, :Cs] and ``d`` = W[:, Cs:], both without affine / ReLU (applied after the interpolation)."""
    def part(cols):
        K, Kpad = cols.shape[1], _round_up(max(cols.shape[1], 1), 16)
        Wp = torch.zeros((first.W.shape[0], Kpad), dtype=torch.float32, device=first.W.device)
        Wp[:, :K] = cols
        return _Layer(W=Wp.contiguous(), scale=torch.ones_like(first.scale), shift=torch.zeros_like(first.shift), N=first.N,
                      K=K, Kpad=Kpad, relu=0)

    def build():
        Cd = first.K - Cs
        wd4 = None
        if 0 < Cd <= 4:   # narrow skip input (rgb): multiplied inside the interpolation kernel
            wd4 = torch.zeros((first.N, 4), dtype=torch.float32, device=first.W.device)
            wd4[:, :Cd] = first.W[:first.N, Cs:first.K]
            wd4 = wd4.contiguous()
        return part(first.W[:, :Cs]), part(first.W[:, Cs:first.K]) if Cd > 4 else None, wd4
    return _derived(first, "fp_split", build)


def _interp_tables(first, wd4):
    """Wd4 (256 x 4) | scale1 (256) | shift1 (256): the tables of fp_head_chain_interp's prologue, cached on the layer."""
    def build():
        wd = wd4 if wd4 is not None else torch.zeros((256, 4), dtype=torch.float32, device=first.W.device)
        return torch.cat([wd.reshape(-1), first.scale[:256], first.shift[:256]]).contiguous()
    return _derived(first, "interp_tables", build)


def interp_affine(Ys, idx, dist2, eps, Yd, dense_small, wd4, layer, B, Ns, Nd):
    """relu(scale * (sum_k w_k Ys[idx_k] + Yd + Wd4 . dense_small) + shift): the 3-NN interpolation of
    pre-multiplied sparse rows.  ``dense_small``: (B,Cd<=4,Nd) any strides, or None."""
    C = layer.N
    out = torch.empty((B * Nd, C), dtype=torch.float32, device=Ys.device)
    dptr, db, dc, dn, Cd = _strided3(dense_small)
    wptr = None if dense_small is None else wd4.data_ptr()
    _call("regnet_interp_affine_f32", Ys, Ys.data_ptr(), Ns * Ys.stride(0), Ys.stride(0), idx.data_ptr(), dist2.data_ptr(),
          float(eps), None if Yd is None else Yd.data_ptr(), 0 if Yd is None else Yd.stride(0), dptr, db, dn, dc, Cd, wptr,
          layer.scale.data_ptr(), layer.shift.data_ptr(), layer.relu, B, Nd, C, out.data_ptr(), out.stride(0))
    return out


def _packed_head(seg):
    """conv_score weight + folded bn_score scalars, cached like the layer stacks (reading the
    scalars costs a device sync, so do it once per weight version, not per forward)."""
    def build():
        conv, bn = seg.conv_score, seg.bn_score
        w = conv.weight.detach().reshape(-1).float().contiguous()
        bn_scale = float(bn.weight.detach()[0] / torch.sqrt(bn.running_var.detach()[0] + bn.eps))
        bn_shift = float(bn.bias.detach()[0] - bn.running_mean.detach()[0] * bn_scale)
        bias = float(conv.bias.detach()[0]) if conv.bias is not None else 0.0
        return w, bias, bn_scale, bn_shift
    return _cached(seg, "score_head", _signature(seg.conv_score) + _signature(seg.bn_score), build)


def score_head(x, seg, P):
    w, bias, bn_scale, bn_shift = _packed_head(seg)
    score = torch.empty((P,), dtype=torch.float32, device=x.device)
    _call("regnet_score_head_f32", x, x.data_ptr(), x.stride(0), w.numel(), w.data_ptr(), bias, bn_scale, bn_shift,
          score.data_ptr(), P)
    return score


def _flop_meta(P, K, N):
    return "P%d K%d N%d flop%d" % (P, K, N, 2 * P * K * N)


# what bench.py brackets with HIP events: name -> meta(args) (algorithmic flops use the TRUE K)
TIMED_OPS = {
    "mlp_layer": lambda A, Ka, layer, P, pool_group=0: _flop_meta(P, layer.K, layer.N) + (" pool%d" % pool_group if pool_group else ""),
    "sa_layer1": lambda feature, xyz, nbr, ctr, layer, B, M, group: _flop_meta(B * M * group, layer.K, layer.N),
    "sa_premul_layer": lambda U, V, nbr, layer, B, Nsrc, M, group, pool_group=0:
        _flop_meta(B * M * group, layer.K, layer.N),
    "sa_chain3": lambda feature, xyz, nbr, ctr, l1, l2, l3, B, M, group, count=None, order=None:
        "P%d K%d N%d flop%d" % (B * M * group, l3.K, l3.N,
                                2 * B * M * group * (l1.K * l1.N + l2.K * l2.N + l3.K * l3.N)),
    "sa_premul_chain": lambda U, V, nbr, module, layers, B, Nsrc, M:
        "P%d K256 N512 flop%d" % (B * M * 64, 2 * B * M * 64 * (256 * 256 + 256 * 512)),
    "sa3_premul_chain": lambda U, V, nbr, module, layers, B, Nsrc, M:
        "P%d K512 N1024 flop%d" % (B * M * 64, 2 * B * M * 64 * (512 * 512 + 512 * 1024)),
    "fp_head_chain_interp": lambda Ys, idx, dist2, eps, dense_small, wd4, first, seg, fp_layers, B, Ns, Nd:
        "P%d K256 N256 flop%d" % (B * Nd, 2 * B * Nd * 491520),
    "fp_head_chain": lambda h1, seg, fp_layers, P: "P%d K256 N256 flop%d" % (P, 2 * P * 491520),
    "sa_layer12": lambda feature, xyz, nbr, ctr, first, layer, B, M, group, pool_group=0:
        "P%d K%d N%d flop%d" % (B * M * group, layer.K, layer.N,
                                2 * B * M * group * (layer.K * layer.N + first.K * first.N)),
}


def _as_channels_last(feature):
    """(B,C,N) tensor -> (B,N,C) contiguous view/copy with channel stride 1."""
    cl = feature.transpose(1, 2)
    return cl if cl.is_contiguous() else cl.contiguous()


# ---- block-level forwards ---------------------------------------------------------------------
# Every block is split into its GEOMETRY part (indices; depends on xyz only) and its FEATURE part
# (the MLP chain).  Called back to back they are the module forward; pipeline.ForwardPipeline runs
# the geometry of batch i+1 on another stream while the features of batch i are on the matrix cores.
def sa_sample(module, xyz, prefix_ok=None):
    """Furthest point sampling of a PointNetSAModule (modules.py:23-26): the long latency chain.  -> (ctr, first_tie).
    ``prefix_ok``: the ``first_tie`` of the sampling run that produced ``xyz``'s ORDER when ``xyz`` is the previous level's
    centroids in pick order (never anything else): scenes whose run had no tie among its first M picks then get 0 .. M-1
    without sampling -- the same indices the sampling would return (pn2_ext.FpsChain, csrc/geometry.hip)."""
    chain = pn2_ext.FpsChain(prefix_ok if FPS_CHAIN else None)
    ctr = pn2_ext.farthest_point_sample(xyz, module.num_centroids, chain)
    return ctr, chain.first_tie


def sa_group(module, xyz, ctr, first_tie=None):
    """Centroid gather + ball query given the sampled indices (modules.py:41, :238-239).  ``first_tie``: of the run that
    sampled ``ctr`` (kept in the plan: the next level's ``prefix_ok``)."""
    B, M = ctr.shape
    new_xyz = pn2_ext.gather_points(xyz, ctr) if xyz.dtype == torch.float32 else torch.gather(xyz, 2, ctr[:, None, :].expand(B, 3, M))
    nbr, count = pn2_ext.ball_query(xyz, new_xyz, module.grouper.radius, module.grouper.num_neighbours)
    geo = {"ctr": ctr, "new_xyz": new_xyz, "nbr": nbr}
    if first_tie is not None:
        geo["first_tie"] = first_tie
    route = sa_route(module)
    prepare = route.prepare if route is not None else None
    if prepare == "pairs":
        # partners whose remainders fit one point tile at waves w and w + 4 of a workgroup (csrc/sa_chain.hip), pairs of 1, 2,
        # 3, 4 tiles in that order so that whole workgroups are of one kind; off the matrix cores' critical path
        geo["count"] = count
        geo["order"] = chain3_pair_order(count)
    elif prepare == "premul":
        # what the pre-multiplied first layer takes from the coordinates only, off the feature stage's stream (a reduction, a
        # pack and a tiny GEMM per level)
        _, (_, v_layer) = _sa_packs(module, route, module.mlp[0].conv.in_channels - 3, xyz.device)
        geo.update(_premul_centres(xyz, new_xyz, v_layer))
    return geo


def sa_geometry(module, xyz, ctr=None, prefix_ok=None):
    """FPS + centroid gather + ball query of a PointNetSAModule.  ``prefix_ok``: see sa_sample (``xyz`` must then be the
    previous level's ``new_xyz``)."""
    if ctr is not None:
        return sa_group(module, xyz, ctr)
    ctr, first_tie = sa_sample(module, xyz, prefix_ok)
    return sa_group(module, xyz, ctr, first_tie)


def sa_features(module, xyz, feature, geo):
    """Grouping + SharedMLP + max over K of a PointNetSAModule (modules.py:44-56, :244-245)."""
    B, N1 = xyz.shape[0], xyz.shape[2]
    M, K = module.num_centroids, module.grouper.num_neighbours
    Cf = 0 if feature is None else feature.size(1)
    route = sa_route(module, feature is not None)
    if route is None:
        raise NotImplementedError("fused SA supports 64 neighbours, >= 2 MLP layers and features only with use_xyz")
    layers, premul = _sa_packs(module, route, Cf, xyz.device)
    P = B * M * K
    pool = 0 if route.tail else K       # no plain layer behind the route's kernel: it takes the max over the neighbours itself
    nbr, ctr = geo["nbr"], geo["ctr"]
    if premul is not None:
        u_layer, v_layer = premul
        if geo.get("V_layer") is not v_layer:    # stale: the weights moved after the plan was made (or it was made for another route)
            geo = dict(geo, **_premul_centres(xyz, geo["new_xyz"], v_layer, geo))
        width = _round_up(Cf + 3, 4)
        U = mlp_layer(pack_rows(feature, xyz, width, geo["mu"]), width, u_layer, B * N1)
    if route.features == "chain3":
        h = sa_chain3(feature, xyz, nbr, ctr, layers[0], layers[1], layers[2], B, M, K, geo.get("count"), geo.get("order"))
    elif route.features == "layer12":
        h = sa_layer12(feature, xyz, nbr, ctr, layers[0], layers[1], B, M, K, pool_group=pool)
    elif route.features == "premul_chain512":   # 512-wide activations (layer 2 as two K-halves)
        h = sa3_premul_chain(U, geo["V"], nbr, module, layers, B, N1, M)
    elif route.features == "premul_chain256":   # the layer-2 activation in registers
        h = sa_premul_chain(U, geo["V"], nbr, module, layers, B, N1, M)
    elif route.features == "premul_layer":
        h = sa_premul_layer(U, geo["V"], nbr, layers[1], B, N1, M, K, pool_group=pool)
    else:
        h = sa_layer1(feature, xyz, nbr, ctr, layers[0], B, M, K)
    for i, layer in enumerate(layers[len(layers) - route.tail:], 1):
        h = mlp_layer(h, layer.K, layer, P, pool_group=K if i == route.tail else 0)
    return geo["new_xyz"], h.view(B, M, -1).transpose(1, 2)              # (B*M, C_out) pooled rows


def sa_forward(module, xyz, feature, geo=None):
    """PointNetSAModule.forward (modules.py:210-246) for num_centroids > 0 with a ball grouper."""
    return sa_features(module, xyz, feature, geo if geo is not None else sa_geometry(module, xyz))


def fp_geometry(module, dense_xyz, sparse_xyz):
    """3-NN search of a PointnetFPModule (modules.py:115-116)."""
    idx, dist2 = pn2_ext.point_search(dense_xyz, sparse_xyz, module.interpolator.num_neighbors)
    return {"idx": idx, "dist2": dist2}


def _fp_route_of(module, dense_xyz, dense_feature, sparse_feature, seg=None):
    return fp_route(module, sparse_feature.size(1), 0 if dense_feature is None else dense_feature.size(1),
                    sparse_feature.size(2), dense_xyz.size(2), seg=seg,
                    f32=dense_feature is None or dense_feature.dtype == torch.float32)


def _fp_packs(module, route, Cs):
    """The packs ``route``'s kernels read (beside the head chain's own, _head_chain_packs): -> (layers, _fp_split_layers or None)."""
    layers = _packed_stack(module, module.mlp)
    return layers, _fp_split_layers(layers[0], Cs) if route.features != "concat" else None


def _fp_first_layer(module, route, layers, split, dense_feature, sparse_feature, geo, seg=None):
    """First layer of a feature-propagation block evaluated on the SPARSE rows (fp_route: every route but concat); -> (B*Nd,
    C1) channels-last activation after BN + ReLU -- route head_interp: -> (F, score) of the whole block and the head."""
    B, Cs, Ns = sparse_feature.shape
    Nd = geo["idx"].size(1)
    lay_s, lay_d, wd4 = split
    Ys = mlp_layer(_as_channels_last(sparse_feature).view(B * Ns, Cs), Cs, lay_s, B * Ns)
    dense_small = dense_feature if route.skip == "table" else None
    if route.features == "head_interp":    # the interpolation inside the chain's prologue
        return fp_head_chain_interp(Ys, geo["idx"], geo["dist2"], module.interpolator._eps, dense_small, wd4, layers[0], seg,
                                    layers, B, Ns, Nd)
    Yd = None
    if route.skip == "gemm":
        Cd = dense_feature.size(1)
        Yd = mlp_layer(_as_channels_last(dense_feature).view(B * Nd, Cd), Cd, lay_d, B * Nd)
    return interp_affine(Ys, geo["idx"], geo["dist2"], module.interpolator._eps, Yd, dense_small, wd4, layers[0], B, Ns, Nd)


def fp_features(module, dense_xyz, dense_feature, sparse_feature, geo):
    """Interpolate + concat + SharedMLP of a PointnetFPModule (modules.py:117-131, :507)."""
    B, _, Nd = dense_xyz.shape
    route = _fp_route_of(module, dense_xyz, dense_feature, sparse_feature)
    layers, split = _fp_packs(module, route, sparse_feature.size(1))
    if route.features == "premul":
        h = _fp_first_layer(module, route, layers, split, dense_feature, sparse_feature, geo)
        Ka, layers = layers[0].N, layers[1:]
    else:
        h, Ka = interp_concat(_as_channels_last(sparse_feature), geo["idx"], geo["dist2"], module.interpolator._eps,
                              dense_feature, B, Nd)
    for layer in layers:
        h = mlp_layer(h, Ka, layer, B * Nd)
        Ka = layer.N
    return h.view(B, Nd, -1).transpose(1, 2)


def fp_forward(module, dense_xyz, sparse_xyz, dense_feature, sparse_feature, geo=None):
    """PointnetFPModule.forward with a 3-NN interpolator (modules.py:104-131, :500-509)."""
    if geo is None:
        geo = fp_geometry(module, dense_xyz, sparse_xyz)
    return fp_features(module, dense_xyz, dense_feature, sparse_feature, geo)


def head_forward(seg, sparse_feature):
    """PointNet2Seg head (pointnet2.py:116-119): SharedMLP -> conv_score -> bn_score -> sigmoid -> (B,N)."""
    B, C, N = sparse_feature.shape
    layers = _packed_stack(seg.mlp, seg.mlp)
    h = _as_channels_last(sparse_feature).view(B * N, C)
    Ka = C
    if Ka % 4:
        raise NotImplementedError("head input width must be a multiple of 4")
    for layer in layers:
        h = mlp_layer(h, Ka, layer, B * N)
        Ka = layer.N
    return score_head(h, seg, B * N).view(B, N)


# ---- level-2 / level-3 set-abstraction blocks: layers 2 + 3 + pooling as ONE kernel (csrc/rowchain.hip) ----------------
_CHAIN_WIDTH = {"premul_chain256": 256, "premul_chain512": 512}    # sa_route -> C, the width of its chain's activations
# C -> (cache slot, launching entry point, the query of its weight stream's size)
_CHAINS = {256: ("sa_chain", "regnet_sa_premul_chain_f32", "regnet_sa_premul_chain_stream_floats"),
           512: ("sa3_chain", "regnet_sa3_premul_chain_f32", "regnet_sa3_premul_chain_stream_floats")}


def _packed_premul_chain(module, layers, C):
    """Weight stream of [32 rows][256 k] stages + affine table of the SA chain with C-wide activations.  Level 2: 24 stages,
    layer 2 then layer 3.  Level 3: 96 stages, W2 as (K-half, 16 row blocks), W3 as (32 row blocks, K-half)."""
    slot, _, stream_floats = _CHAINS[C]

    def build():
        l2, l3 = layers[1], layers[2]
        halves = range(C // 256)
        stages = [_swizzle_stage(l2.W[32 * rg:32 * rg + 32, 256 * kh:256 * kh + 256]) for kh in halves for rg in range(C // 32)]
        stages += [_swizzle_stage(l3.W[32 * s:32 * s + 32, 256 * kh:256 * kh + 256]) for s in range(C // 16) for kh in halves]
        stream = torch.cat(stages).contiguous()
        affine = torch.cat([l2.scale[:C], l2.shift[:C], l3.scale[:2 * C], l3.shift[:2 * C]]).contiguous()
        assert stream.numel() == getattr(_L, stream_floats)() and affine.numel() == 6 * C
        return stream, affine
    return _cached(module, slot, _signature(module.mlp), build)


def _premul_chain(C, U, V, nbr, module, layers, B, Nsrc, M):
    stream, affine = _packed_premul_chain(module, layers, C)
    out = torch.empty((B * M, 2 * C), dtype=torch.float32, device=U.device)
    ticket = _tickets(U.device)
    _call(_CHAINS[C][1], U, U.data_ptr(), U.stride(0), V.data_ptr(), V.stride(0), nbr.data_ptr(), B, Nsrc, M, stream.data_ptr(),
          stream.numel() // 8192, affine.data_ptr(), affine.numel(), layers[2].relu, out.data_ptr(), out.stride(0),
          ticket.data_ptr())
    return out


def sa_premul_chain(U, V, nbr, module, layers, B, Nsrc, M):
    """relu(U[nbr] - V[centre]) -> 256 -> 512 -> max over the 64 neighbours, one launch; -> (B*M, 512)."""
    return _premul_chain(256, U, V, nbr, module, layers, B, Nsrc, M)


def sa3_premul_chain(U, V, nbr, module, layers, B, Nsrc, M):
    """relu(U[nbr] - V[centre]) -> 512 -> 1024 -> max over the 64 neighbours, one launch; -> (B*M, 1024)."""
    return _premul_chain(512, U, V, nbr, module, layers, B, Nsrc, M)


# ---- FP3 tail + segmentation head as ONE kernel (csrc/rowchain.hip) --------------------------------------------------
def _swizzle_stage(block):
    """(R, KC) weight block -> the LDS image of a rowchain stage: 16-byte chunk c' of row r holds logical chunk
    c' ^ (r & 15) (XOR on the low 4 bits of the chunk index; see csrc/rowchain.hip:rc_frag_offsets)."""
    R, KC = block.shape
    chunks = block.reshape(R, KC // 4, 4)
    r = torch.arange(R, device=block.device)[:, None]
    cp = torch.arange(KC // 4, device=block.device)[None, :]
    src = (cp & ~15) | ((cp ^ r) & 15)
    return chunks.gather(1, src[:, :, None].expand(R, KC // 4, 4)).reshape(-1)


def _rowchain_pair_stream(la, lb):
    """Stream of one layer pair (A: 256 -> M, B: M -> N) in consumption order: per 128-channel group of M, four
    A-stages [32 rows][256 k] then N/64 B-stages [64 rows][128 k]."""
    WA, WB = la.W[:la.N, :la.K], lb.W[:lb.N, :lb.K]
    M, N = la.N, lb.N
    assert la.K == 256 and lb.K == M and M % 128 == 0 and N % 64 == 0
    out = []
    for ob in range(M // 128):
        for u in range(4):
            out.append(_swizzle_stage(WA[128 * ob + 32 * u:128 * ob + 32 * u + 32, :]))
        for v in range(N // 64):
            out.append(_swizzle_stage(WB[64 * v:64 * v + 64, 128 * ob:128 * ob + 128]))
    return out


def _packed_rowchain(seg, fp_layers):
    """Weight stream + affine table of the FP3-tail + head chain, cached on ``seg`` per weight version."""
    layers = list(fp_layers[1:]) + list(_packed_stack(seg.mlp, seg.mlp))

    def build():
        stages = []
        for a, b in ((layers[0], layers[1]), (layers[2], layers[3]), (layers[4], layers[5])):
            stages += _rowchain_pair_stream(a, b)
        stream = torch.cat(stages).contiguous()
        affine = torch.cat([torch.cat([L.scale[:L.N], L.shift[:L.N]]) for L in layers]).contiguous()
        assert stream.numel() == _L.regnet_fp_head_chain_stream_floats() and affine.numel() == 3328
        return stream, affine
    return _cached(seg, "rowchain", _signature(seg.fp_modules[-1]) + _signature(seg.mlp), build)


def supports_rowchain(seg, fp_module):
    """The chained kernel covers exactly the reference's configuration (pointnet2.py:44-46): FP channels
    (256, 256, 256) and head channels (512, 256, 256, 128) with ReLU everywhere, one score channel."""
    if not ROWCHAIN or seg.k_score != 1:
        return False
    widths = [b.conv.out_channels for b in fp_module.mlp] + [b.conv.out_channels for b in seg.mlp]
    relus = [b.relu is not None and b.bn is not None for b in list(fp_module.mlp) + list(seg.mlp)]
    return widths == [256, 256, 256, 512, 256, 256, 128] and all(relus) and seg.mlp[0].conv.in_channels == 256


def _head_chain_packs(seg, fp_layers, first=None, wd4=None):
    """The head routes' own packs: -> (weight stream, affine table, score head, head_interp's tables -- given its ``first`` layer)."""
    return (*_packed_rowchain(seg, fp_layers), _packed_head(seg), None if first is None else _interp_tables(first, wd4))


def fp_head_chain(h1, seg, fp_layers, P):
    """h1 (P, 256) -> (F (P, 256), score (P,)): FP layers 2-3 and the segmentation head in one launch."""
    stream, affine, (w, bias, bn_scale, bn_shift), _ = _head_chain_packs(seg, fp_layers)
    F = torch.empty((P, 256), dtype=torch.float32, device=h1.device)
    score = torch.empty((P,), dtype=torch.float32, device=h1.device)
    ticket = _tickets(h1.device)   # work-queue head, zeroed on this stream
    _call("regnet_fp_head_chain_f32", h1, h1.data_ptr(), h1.stride(0), stream.data_ptr(), 60, affine.data_ptr(),
          affine.numel(), w.data_ptr(), bias, bn_scale, bn_shift, F.data_ptr(), F.stride(0), score.data_ptr(), P,
          ticket.data_ptr(), 0, -1)
    return F, score


TAIL_SINK = None       # a list (set by ForwardPipeline around a feature stage): fp_head_chain_interp puts its partial last round
                        # of blocks on a side stream and appends the event that marks its end; None: one launch, as always
_CUS = 256
_tail_streams = {}


def _tail_stream(device):
    key = device.index if device.index is not None else torch.cuda.current_device()
    if key not in _tail_streams:
        _tail_streams[key] = torch.cuda.Stream(device)
    return _tail_streams[key]


def fp_head_chain_interp(Ys, idx, dist2, eps, dense_small, wd4, first, seg, fp_layers, B, Ns, Nd):
    """(Ys (B*Ns, 256) pre-multiplied sparse rows, 3-NN indices / squared distances, rgb-like skip input) -> (F, score):
    the whole last feature-propagation block + the segmentation head in one launch; h1 is never written."""
    stream, affine, (w, bias, bn_scale, bn_shift), tables = _head_chain_packs(seg, fp_layers, first, wd4)
    P = B * Nd
    F = torch.empty((P, 256), dtype=torch.float32, device=Ys.device)
    score = torch.empty((P,), dtype=torch.float32, device=Ys.device)
    tickets = _tickets(Ys.device, 2)
    dptr, db, dc, dn, Cd = _strided3(dense_small)

    def launch(first, count, ticket, stream_handle=None):
        _call("regnet_fp_head_chain_interp_f32", Ys, Ys.data_ptr(), Ns * Ys.stride(0), Ys.stride(0), idx.data_ptr(),
              dist2.data_ptr(), float(eps), dptr, db, dn, dc, Cd, tables.data_ptr(), B, Nd, stream.data_ptr(), 60,
              affine.data_ptr(), affine.numel(), w.data_ptr(), bias, bn_scale, bn_shift, F.data_ptr(), F.stride(0),
              score.data_ptr(), ticket.data_ptr(), first, count, stream=stream_handle)

    # The last round of 128-row blocks is partial (8 x 25 600 rows: 1600 blocks = 6 x 256 + 64): run alone it keeps 64 CUs
    # busy for a whole pass while 192 idle (a pass costs the same however few blocks it holds).  A caller that can run
    # something else meanwhile -- ForwardPipeline: the NEXT batch's first kernels -- collects it from TAIL_SINK: the tail
    # goes to a side stream behind the inputs, and the caller orders the consumers of F / score behind the event it gets.
    blocks = _L.regnet_fp_head_chain_blocks(P)
    tail = blocks % _CUS
    if TAIL_SINK is not None and blocks > _CUS and 0 < tail <= _CUS // 2:
        # (no device context: an event binds to the device of the stream that first records it, the side stream is created
        # for Ys.device by name)
        cur = torch.cuda.current_stream(Ys.device)
        side = _tail_stream(Ys.device)
        ready = torch.cuda.Event()
        ready.record(cur)
        side.wait_event(ready)
        launch(blocks - tail, tail, tickets[1:], side.cuda_stream)
        done = torch.cuda.Event()
        done.record(side)
        for t in (Ys, idx, dist2, tables, stream, affine, w, F, score, tickets) + (() if dense_small is None else (dense_small,)):
            t.record_stream(side)
        TAIL_SINK.append(done)
        launch(0, blocks - tail, tickets[:1], cur.cuda_stream)
    else:
        launch(0, -1, tickets[:1])
    return F, score


def fp_head_forward(seg, fp_module, dense_xyz, dense_feature, sparse_feature, geo):
    """Last feature-propagation block + segmentation head (pointnet2.py:64-84, :116-119) -> (feature (B,256,N) view,
    score (B,N)); None when the chained kernel does not apply (the caller then runs the two blocks separately)."""
    route = _fp_route_of(fp_module, dense_xyz, dense_feature, sparse_feature, seg)
    if route is None:
        return None
    B, _, Nd = dense_xyz.shape
    layers, split = _fp_packs(fp_module, route, sparse_feature.size(1))
    out = _fp_first_layer(fp_module, route, layers, split, dense_feature, sparse_feature, geo, seg)
    F, score = out if route.features == "head_interp" else fp_head_chain(out, seg, layers, B * Nd)
    return F.view(B, Nd, 256).transpose(1, 2), score.view(B, Nd)


def prepack(score_net, region_net=None):
    """Build every packed-weight cache of the fused forward NOW, on the current stream: the packs of the route each block will
    take, through the helpers its kernels read them through.  The caches are otherwise filled lazily by whichever stream first
    runs a block; with several feature-stage streams (``ForwardPipeline(mlp_streams=2)``) a second stream could then read a
    cache whose packing kernels, enqueued on the first, have not finished.  ``ForwardPipeline.run`` calls this first."""
    forget(score_net, region_net)
    seg = getattr(score_net, "extrat_featurePN2", score_net)
    dev = next(seg.parameters()).device
    for sa in seg.sa_modules:
        route = sa_route(sa, bool(sa.in_channels))
        if route is not None:
            layers, premul = _sa_packs(sa, route, sa.in_channels, dev)
            if route.features in _CHAIN_WIDTH:
                _packed_premul_chain(sa, layers, _CHAIN_WIDTH[route.features])
    Cs = seg.sa_modules[-1].out_channels
    for fp in seg.fp_modules:
        last = fp is seg.fp_modules[-1]
        Cd = fp.mlp[0].conv.in_channels - Cs
        route = (fp_route(fp, Cs, Cd, seg=seg) if last else None) or fp_route(fp, Cs, Cd)
        layers, split = _fp_packs(fp, route, Cs)
        if route.features.startswith("head"):
            _head_chain_packs(seg, layers, *((layers[0], split[2]) if route.features == "head_interp" else ()))
        Cs = fp.out_channels
    _packed_stack(seg.mlp, seg.mlp)
    _packed_head(seg)
    if region_net is not None:
        _packed_named(region_net.extrat_feature_region, _TWOSTAGE, _TWOSTAGE_TREE)
        _packed_named(region_net.extrat_feature_refine, _REFINE, _REFINE_TREE)


def plan_tensors(plan):
    """All tensors of a geometry plan (for Tensor.record_stream when it crosses streams)."""
    out = []
    for level in plan["sa"] + plan["fp"]:
        out.extend(v for v in level.values() if isinstance(v, torch.Tensor))
    return out


# ---- grasp-region / refine heads (tiny GEMMs: P = #centres; kept on the same kernel so the whole
#      forward is deterministic and independent of the torch convolution backend) -----------------
def _packed_named(net, names, tree):
    """names: list of (conv_attr, bn_attr, relu).  Cached on ``net`` like the SharedMLP stacks.  ``tree``: (trunk, (a, b)) of
    heads_tree_kernel (see _heads_tree); when the layers' shapes suit that kernel, the pack also holds the two branches'
    first layers a and b as ONE layer under the key (a, b): weights and folded BatchNorm concatenated row-wise."""
    def build():
        L = {c: _pack(getattr(net, c), getattr(net, bn), relu) for c, bn, relu in names}
        trunk, (a, b) = tree
        la, lb, lt = L[a], L[b], L[trunk]
        if (lt.N % 256 == 0 and la.K == lb.K == lt.N and la.relu == lb.relu and la.N % 16 == 0
                and la.N + lb.N in (256, 512)):
            L[a, b] = _Layer(W=torch.cat([la.W[:la.N], lb.W[:lb.N]]), scale=torch.cat([la.scale, lb.scale]),
                             shift=torch.cat([la.shift, lb.shift]), N=la.N + lb.N, K=la.K, Kpad=la.Kpad, relu=la.relu)
        return L
    return _cached(net, "heads", _signature(net), build)


_TWOSTAGE = [("conv", "bn", True), ("conv_cls2", "bn_cls2", True), ("conv_cls3", "bn_cls3", True),
             ("conv_cls4", "bn_cls4", False), ("conv_reg2", "bn_reg2", True), ("conv_reg3", "bn_reg3", True),
             ("conv_reg4", "bn_reg4", False)]
_REFINE = [("conv_formal", "bn_formal", True), ("conv_formal_cls2", "bn_formal_cls2", True),
           ("conv_formal_cls3", "bn_formal_cls3", False), ("conv_formal_reg2", "bn_formal_reg2", True),
           ("conv_formal_reg3", "bn_formal_reg3", False)]
_TWOSTAGE_TREE = ("conv", ("conv_cls2", "conv_reg2"))
_REFINE_TREE = ("conv_formal", ("conv_formal_cls2", "conv_formal_reg2"))


FPS_CHAIN = True     # levels 2+ hand the level above's sampling certificate down (sa_sample): no sampling unless it had a tie
HEADS_CHAIN = True   # the grasp heads as ONE launch each (csrc/heads.hip) instead of a split-K GEMM + its reduction per layer
# ... up to this many rows.  The one launch is 16 rows per workgroup, each streaming all the head's weights through one CU for
# ~0.1-0.4 ms: the latency win at B <= 4 (<= 256 centres).  At B = 8 its 32 whole-CU workgroups sit under the NEXT batch's SA
# chains and the layer-wise split-K path measured 1 % faster end to end (scripts/ablate/frac_ab.sh, profiles/r04j_heads_ab.txt).
HEADS_CHAIN_MAX_ROWS = 256


def _heads_launch(entry, x, L, rows, count, n_a, n_b):
    """One launch of a csrc/heads.hip entry point on x (n, K) float32 rows -> (out_a (n, n_a), out_b (n, n_b)).  ``rows``:
    [(layer name, *where)] in execution order; the int64 descriptor (device addresses of the packed weights, the layer's
    shape, then ``where``) is built per call."""
    n = x.shape[0]
    x = x if x.stride(1) == 1 and x.stride(0) % 4 == 0 and x.data_ptr() % 16 == 0 else x.contiguous().clone()
    descr = []
    for name, *where in rows:
        lay = L[name]
        descr += [lay.W.data_ptr(), lay.scale.data_ptr(), lay.shift.data_ptr(), lay.K, lay.Kpad, lay.N, lay.relu, *where]
    arr = (ctypes.c_int64 * len(descr))(*descr)
    out_a = torch.empty((n, n_a), dtype=torch.float32, device=x.device)
    out_b = torch.empty((n, n_b), dtype=torch.float32, device=x.device)
    _call(entry, x, x.data_ptr(), x.stride(0), x.shape[1], n, ctypes.addressof(arr), count, out_a.data_ptr(), n_a,
          out_b.data_ptr(), n_b)
    return out_a, out_b


def _heads_chain(x, L, plan, n_a, n_b):
    """``plan``: [(layer name, src buffer, dst buffer)] in execution order (buffers: 0 input, 1-3 LDS scratch, 4 / 5 outputs
    a / b): nine integers per layer."""
    return _heads_launch("regnet_heads_chain_f32", x, L, plan, len(plan), n_a, n_b)


HEADS_TREE = True    # more rows than HEADS_CHAIN_MAX_ROWS: ONE launch of csrc/heads.hip's heads_tree_kernel (32 rows per workgroup,
                     # the trunk activation chunked through LDS) instead of a split-K GEMM + its reduction per layer


def _heads_tree(x, L, tree, tails, n_a, n_b):
    """x (n, K) rows -> (out_a (n, n_a), out_b (n, n_b)) by ``regnet_heads_tree_f32``.  ``tree``: (trunk layer name, the two
    branches' first layer names), whose joined layer ``_packed_named`` put in ``L``; ``tails``: [(layer, src, src_off, dst,
    dst_off)] in execution order."""
    trunk, first = tree
    return _heads_launch("regnet_heads_tree_f32", x, L, [(trunk, 0, 0, 0, 0), (first, 0, 0, 0, 0)] + tails, len(tails), n_a, n_b)


def _tree_ok(L, tree, x):
    return HEADS_TREE and x.shape[1] % 4 == 0 and tree[1] in L


_TWOSTAGE_PLAN = [("conv", 0, 1), ("conv_cls2", 1, 2), ("conv_cls3", 2, 3), ("conv_cls4", 3, 4),
                  ("conv_reg2", 1, 2), ("conv_reg3", 2, 3), ("conv_reg4", 3, 5)]
_REFINE_PLAN = [("conv_formal", 0, 1), ("conv_formal_cls2", 1, 2), ("conv_formal_cls3", 2, 4),
                ("conv_formal_reg2", 1, 2), ("conv_formal_reg3", 2, 5)]


def _chain(x, layers, names):
    P = x.shape[0]
    for n in names:
        x = mlp_layer(x, layers[n].K, layers[n], P)
    return x


def twostage_forward(net, mp_x, raw_reg=False):
    """PointNet2TwoStage.forward after the max-pool (pointnet2.py:174-188): mp_x (n, 256, 1) ->
    x_cls (n, k_cls), x_reg (n, k_cls, k_reg/k_cls) with sigmoid on channels 7: (``raw_reg``: without it -- the caller's
    decode kernel applies it to the one anchor it keeps, region_ops.stage2_decode)."""
    n = mp_x.shape[0]
    L = _packed_named(net, _TWOSTAGE, _TWOSTAGE_TREE)
    x = mp_x.reshape(n, -1).contiguous()
    if HEADS_CHAIN and n <= HEADS_CHAIN_MAX_ROWS and x.shape[1] % 16 == 0:
        x_cls, x_reg = _heads_chain(x, L, _TWOSTAGE_PLAN, L["conv_cls4"].N, L["conv_reg4"].N)
    elif _tree_ok(L, _TWOSTAGE_TREE, x) and L["conv_cls3"].K == L["conv_cls2"].N:
        n2, n3 = L["conv_cls2"].N, L["conv_cls3"].N
        x_cls, x_reg = _heads_tree(x, L, _TWOSTAGE_TREE,
                                   [("conv_cls3", 0, 0, 1, 0), ("conv_reg3", 0, n2, 1, _round_up(n3, 16)),
                                    ("conv_cls4", 1, 0, 4, 0), ("conv_reg4", 1, _round_up(n3, 16), 5, 0)],
                                   L["conv_cls4"].N, L["conv_reg4"].N)
    else:
        h = mlp_layer(x, L["conv"].K, L["conv"], n)
        x_cls = _chain(h, L, ["conv_cls2", "conv_cls3", "conv_cls4"])
        x_reg = _chain(h, L, ["conv_reg2", "conv_reg3", "conv_reg4"])
    x_reg = x_reg.view(n, -1, net.k_reg_no_anchor)
    if not raw_reg:
        x_reg[:, :, 7:] = torch.sigmoid(x_reg[:, :, 7:])
    return x_cls, x_reg


def refine_forward(net, x):
    """PointNet2Refine.forward after pooling + concat (pointnet2.py:240-253): x (n, 384, 1) ->
    x_cls (n, 2), x_reg (n, k_reg)."""
    n = x.shape[0]
    L = _packed_named(net, _REFINE, _REFINE_TREE)
    if HEADS_CHAIN and n <= HEADS_CHAIN_MAX_ROWS and (x.numel() // max(n, 1)) % 16 == 0:
        return _heads_chain(x.reshape(n, -1), L, _REFINE_PLAN, L["conv_formal_cls3"].N, L["conv_formal_reg3"].N)
    rows = x.reshape(n, -1)
    if _tree_ok(L, _REFINE_TREE, rows):
        n2 = L["conv_formal_cls2"].N
        return _heads_tree(rows, L, _REFINE_TREE,
                           [("conv_formal_cls3", 0, 0, 4, 0), ("conv_formal_reg3", 0, n2, 5, 0)],
                           L["conv_formal_cls3"].N, L["conv_formal_reg3"].N)
    h = mlp_layer(x.reshape(n, -1).contiguous(), L["conv_formal"].K, L["conv_formal"], n)
    return (_chain(h, L, ["conv_formal_cls2", "conv_formal_cls3"]),
            _chain(h, L, ["conv_formal_reg2", "conv_formal_reg3"]))
