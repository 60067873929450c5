"""The case table of the fused eval-mode forward (regnet_for_3d_grasping_amd/fused.py): which kernels a set-abstraction or a
feature-propagation block of a given description runs on under given module switches.  Every expectation is written by hand
from the rules in ``sa_route`` / ``fp_route``'s documentation, never computed by calling them; tests/test_fused_route_cpu.py
holds the two functions against the table and tests/test_gpu_fused_route.py holds the launches of a real forward against them.

A set-abstraction row is ``Sa(Cf, widths, switches, expect, relu, neighbours, use_xyz, has_feature, mode)``:
  Cf           feature channels: the first convolution reads Cf + 3 ([xyz | feature], use_xyz) -- 0 with has_feature False
  widths       output channels of the MLP layers
  switches     overrides of fused.py's upper-case switches
  expect       (features, tail, prepare), or None for a block the fused forward does not cover
  relu         per layer, None: everywhere (only such a row can be a real PointNetSAModule; the others are stand-ins)
  mode         "eval" (no autograd) | "train" (module.training) | "grad" (eval mode under autograd)
A feature-propagation row is ``Fp(Cs, Cd, widths, switches, expect, Ns, Nd, seg, f32)``:
  Cs, Cd       channels of the sparse and of the dense (skip) input; the first convolution reads Cs + Cd
  Ns, Nd       their points; None, None: the caller knows widths only
  seg          None, or the k_score of the PointNet2Seg whose last block this is (routed with ``seg``)
  expect       (features, skip), or None where block + head as one kernel does not apply
The limits in the comments are those of csrc/mlp.hip, csrc/sa_chain.hip and csrc/rowchain.hip: the gather-fused first layer
takes at most 8 input channels and a first width that is a multiple of 16; sa_chain3 is built for 128 -> 128 -> a multiple of
32; the two pre-multiplied chains for 256 -> 256 -> 512 and 512 -> 512 -> 1024; interp_affine walks a row with C1 / 4 lanes
and a block of 256 holds a whole number of rows; the head chain is the reference's (256, 256, 256) + (512, 256, 256, 128).
"""
import collections
import contextlib
import functools
import types

Sa = collections.namedtuple("Sa", "Cf widths switches expect relu neighbours use_xyz has_feature mode")
Fp = collections.namedtuple("Fp", "Cs Cd widths switches expect Ns Nd seg f32")

SA_FIELDS = ("features", "tail", "prepare")
SA_VALUES = {"features": {"chain3", "layer12", "premul_chain512", "premul_chain256", "premul_layer", "layer1"},
             "tail": {0, 1, 2}, "prepare": {None, "pairs", "premul"}}
FP_FIELDS = ("features", "skip")
FP_VALUES = {"features": {"head_interp", "head_chain", "premul", "concat"}, "skip": {None, "table", "gemm"}}
SWITCHES = ("CHAIN3", "PREMUL", "ROWCHAIN", "SA3_CHAIN", "FP_HEAD_INTERP")

SA1, SA2, SA3 = (128, 128, 256), (256, 256, 512), (512, 512, 1024)        # pointnet2._SA_CHANNELS


def _sa(Cf, widths, expect, relu=None, neighbours=64, use_xyz=True, has_feature=True, mode="eval", **switches):
    return Sa(Cf, widths, switches, expect, relu, neighbours, use_xyz, has_feature, mode)


def _fp(Cs, Cd, widths, expect, Ns=16, Nd=129, seg=None, f32=True, **switches):
    return Fp(Cs, Cd, widths, switches, expect, Ns, Nd, seg, f32)


SA_CASES = [
    # ---- the reference network (pointnet2._SA_CHANNELS), eval / training / eval under autograd ---------------------------------
    _sa(3, SA1, ("chain3", 0, "pairs")),
    _sa(256, SA2, ("premul_chain256", 0, "premul")),
    _sa(512, SA3, ("premul_chain512", 0, "premul")),
    _sa(3, SA1, ("chain3", 0, "pairs"), mode="train"),             # the pairing reads no weight: the same in every mode
    _sa(256, SA2, ("premul_chain256", 0, None), mode="train"),     # V is a function of the weights: the eval forward only
    _sa(512, SA3, ("premul_chain512", 0, None), mode="train"),
    _sa(3, SA1, ("chain3", 0, "pairs"), mode="grad"),
    _sa(256, SA2, ("premul_chain256", 0, None), mode="grad"),
    _sa(512, SA3, ("premul_chain512", 0, None), mode="grad"),
    # ---- one switch each, on a block it serves and on one it does not ---------------------------------------------------------
    _sa(3, SA1, ("layer12", 1, None), CHAIN3=False),
    _sa(256, SA2, ("premul_chain256", 0, "premul"), CHAIN3=False),
    _sa(256, SA2, ("layer1", 2, None), PREMUL=False),
    _sa(512, SA3, ("layer1", 2, None), PREMUL=False),
    _sa(3, SA1, ("chain3", 0, "pairs"), PREMUL=False),
    _sa(256, SA2, ("premul_layer", 1, "premul"), ROWCHAIN=False),
    _sa(512, SA3, ("premul_chain512", 0, "premul"), ROWCHAIN=False),
    _sa(512, SA3, ("premul_layer", 1, "premul"), SA3_CHAIN=False),
    _sa(256, SA2, ("premul_chain256", 0, "premul"), SA3_CHAIN=False),
    _sa(256, SA2, ("premul_chain256", 0, "premul"), FP_HEAD_INTERP=False),     # (a set-abstraction block does not read it)
    # ---- input channels 8 | 9 (Cf 5 | 6): the gather-fused first layer holds its weights as [N][8] ---------------------------
    _sa(5, SA1, ("chain3", 0, "pairs")),
    _sa(6, SA1, ("premul_layer", 1, "premul")),
    _sa(5, (64, 64, 128), ("layer12", 1, None)),
    _sa(6, (64, 64, 128), ("premul_layer", 1, "premul")),
    _sa(6, (64, 64, 128), ("layer1", 2, None), PREMUL=False),
    # ---- first width 40 (no multiple of 16: not the gather-fused layer; a multiple of 4: pre-multiplied, narrow input or
    #      not), 42 (neither), 64, 128; 2-, 3- and 4-layer stacks ------------------------------------------------------------------
    _sa(3, (40, 64), ("premul_layer", 0, "premul")),
    _sa(3, (40, 64), ("layer1", 1, None), PREMUL=False),
    _sa(3, (42, 64), ("layer1", 1, None)),
    _sa(3, (64, 128), ("layer12", 0, None)),
    _sa(3, (64, 64, 128), ("layer12", 1, None)),
    _sa(3, (128, 256), ("layer12", 0, None)),
    _sa(3, (128, 128, 256, 256), ("layer12", 2, None)),            # sa_chain3 is the whole block or nothing
    _sa(3, (128, 128, 240), ("layer12", 1, None)),                 # ... and its last width a multiple of 32
    _sa(3, (128, 64, 256), ("layer12", 1, None)),
    _sa(128, (128, 256), ("premul_layer", 0, "premul")),
    _sa(128, SA1, ("premul_layer", 1, "premul")),
    _sa(128, (128, 256), ("layer1", 1, None), PREMUL=False),
    _sa(128, SA1, ("layer1", 2, None), PREMUL=False),
    _sa(128, SA2, ("premul_chain256", 0, "premul")),               # the chains start behind layer 1: any input width
    _sa(128, (256, 256), ("premul_layer", 0, "premul")),
    _sa(128, (256, 256, 512, 512), ("premul_layer", 2, "premul")),
    _sa(128, (42, 64, 64), ("layer1", 2, None)),
    # ---- a layer without ReLU (stand-ins: a SharedMLP has one everywhere) -----------------------------------------------------------
    _sa(3, SA1, ("layer1", 2, None), relu=(False, True, True)),    # the fused first layers clamp in the operand load
    _sa(256, SA2, ("layer1", 2, None), relu=(False, True, True)),
    _sa(3, SA1, ("layer12", 1, None), relu=(True, False, True)),   # the chains clamp layer 2 in registers
    _sa(256, SA2, ("premul_layer", 1, "premul"), relu=(True, False, True)),
    _sa(512, SA3, ("premul_layer", 1, "premul"), relu=(True, False, True)),
    _sa(3, SA1, ("chain3", 0, "pairs"), relu=(True, True, False)),  # the last layer's ReLU is the kernel's argument
    # ---- no point features: coordinates only ----------------------------------------------------------------------------------------
    _sa(0, SA1, ("chain3", 0, "pairs"), has_feature=False),
    _sa(0, (64, 128), ("layer12", 0, None), has_feature=False),
    _sa(0, (40, 64), ("layer1", 1, None), has_feature=False),      # nothing to pre-multiply per source point
    # ---- what the fused forward does not cover (supports_sa: the operator-granular path) ---------------------------------------
    _sa(3, (32, 64), None, neighbours=32),
    _sa(3, (48,), None),
    _sa(3, SA1, None, use_xyz=False),
]

FP_CASES = [
    # ---- the reference network (pointnet2._FP_CHANNELS): the last block routed with its PointNet2Seg --------------------------
    _fp(1024, 512, (1024, 1024), ("premul", "gemm"), Ns=256, Nd=1024),
    _fp(1024, 256, (512, 512), ("premul", "gemm"), Ns=1024, Nd=5120),
    _fp(512, 3, (256, 256, 256), ("head_interp", "table"), Ns=5120, Nd=25600, seg=1),
    _fp(512, 3, (256, 256, 256), ("premul", "table"), Ns=5120, Nd=25600),      # ... and on its own (add_channel inputs)
    # ---- one switch each --------------------------------------------------------------------------------------------------------
    _fp(512, 3, (256, 256, 256), ("head_chain", "table"), seg=1, FP_HEAD_INTERP=False),
    _fp(512, 3, (256, 256, 256), None, seg=1, ROWCHAIN=False),
    _fp(512, 3, (256, 256, 256), ("premul", "table"), ROWCHAIN=False),
    _fp(512, 3, (256, 256, 256), None, seg=1, PREMUL=False),       # the chain starts from the pre-multiplied first layer
    _fp(512, 3, (256, 256, 256), ("concat", None), PREMUL=False),
    _fp(1024, 256, (512, 512), ("concat", None), PREMUL=False),
    _fp(1024, 256, (512, 512), ("premul", "gemm"), FP_HEAD_INTERP=False),
    _fp(512, 3, (256, 256, 256), ("head_interp", "table"), seg=1, CHAIN3=False),       # (set-abstraction switches: not read)
    _fp(512, 3, (256, 256, 256), ("head_interp", "table"), seg=1, SA3_CHAIN=False),
    # ---- skip channels 0 | 3 | 4 (inside the interpolation) | 6 (neither that nor float4 rows) | 64 (a product of its own) ---
    _fp(256, 0, (256, 128), ("premul", None)),
    _fp(256, 3, (256, 128), ("premul", "table")),
    _fp(256, 4, (256, 128), ("premul", "table")),
    _fp(256, 6, (256, 128), ("concat", None)),
    _fp(256, 64, (256, 128), ("premul", "gemm")),
    _fp(512, 0, (256, 256, 256), ("head_interp", None), seg=1),
    _fp(512, 4, (256, 256, 256), ("head_interp", "table"), seg=1),
    _fp(512, 6, (256, 256, 256), None, seg=1),
    _fp(512, 64, (256, 256, 256), ("head_chain", "gemm"), seg=1),  # the prologue multiplies at most 4 skip channels
    _fp(512, 64, (256, 256, 256), ("head_chain", "gemm"), seg=1, FP_HEAD_INTERP=False),
    # ---- sparse channels no multiple of 4; first widths whose rows do not tile a block of 256 lanes ---------------------------
    _fp(254, 3, (256, 128), ("concat", None)),
    _fp(256, 3, (96, 128), ("concat", None)),                      # 24 lanes per row
    _fp(256, 3, (2048, 128), ("concat", None)),                    # 512 lanes per row
    _fp(256, 3, (1024, 128), ("premul", "table")),
    _fp(256, 3, (30, 128), ("concat", None)),
    # ---- as many sparse points as dense ones, or more: nothing saved; widths only: assumed fewer ----------------------------------
    _fp(256, 3, (256, 128), ("concat", None), Ns=129, Nd=129),
    _fp(256, 3, (256, 128), ("concat", None), Ns=200, Nd=129),
    _fp(512, 3, (256, 256, 256), None, Ns=129, Nd=129, seg=1),
    _fp(256, 3, (256, 128), ("premul", "table"), Ns=None, Nd=None),
    _fp(512, 3, (256, 256, 256), ("head_interp", "table"), Ns=None, Nd=None, seg=1),
    # ---- a float64 skip input; a head the chain is not built for --------------------------------------------------------------------
    _fp(256, 3, (256, 128), ("concat", None), f32=False),
    _fp(512, 3, (256, 256, 256), None, seg=1, f32=False),
    _fp(512, 3, (256, 256, 256), None, seg=2),                     # k_score 2
    _fp(512, 3, (256, 256, 128), None, seg=1),
]


def case_id(case):
    sa = isinstance(case, Sa)
    head = "sa-%d-%s" % (case.Cf, "x".join(map(str, case.widths))) if sa else "fp-%d+%d-%s" % (case.Cs, case.Cd, "x".join(map(str, case.widths)))
    default = _sa(0, (), None) if sa else _fp(0, 0, (), None)
    rest = [(k, v) for k, v, d in zip(case._fields, case, default) if k in ("relu", "neighbours", "use_xyz", "has_feature", "mode",
                                                                              "Ns", "Nd", "seg", "f32") and v != d]
    return head + "".join("-%s=%s" % kv for kv in rest) + "".join("-%s=%d" % kv for kv in sorted(case.switches.items()))


def _blocks(first_in, widths, relu=None):
    """What the routes read of a SharedMLP: per layer the convolution's channel counts and whether BatchNorm / ReLU follow."""
    ins = (first_in,) + tuple(widths[:-1])
    return [types.SimpleNamespace(conv=types.SimpleNamespace(in_channels=i, out_channels=o), bn=object(),
                                  relu=object() if relu is None or relu[k] else None)
            for k, (i, o) in enumerate(zip(ins, widths))]


def sa_stand_in(case):
    """What ``sa_route`` reads of a PointNetSAModule, without its weights."""
    return types.SimpleNamespace(mlp=_blocks(case.Cf + (3 if case.use_xyz else 0), case.widths, case.relu), training=case.mode == "train",
                                 use_xyz=case.use_xyz, grouper=types.SimpleNamespace(num_neighbours=case.neighbours))


def sa_module(case):
    """The real module of the row's description, or None for a row only a stand-in can describe."""
    from regnet_for_3d_grasping_amd.pn2_utils.modules import PointNetSAModule
    if case.relu is not None:
        return None
    return PointNetSAModule(case.Cf, case.widths, 16, 0.1, case.neighbours, case.use_xyz).train(case.mode == "train")


def fp_stand_in(case):
    """What ``fp_route`` reads of a PointnetFPModule and of its PointNet2Seg: -> (module, seg or None)."""
    module = types.SimpleNamespace(mlp=_blocks(case.Cs + case.Cd, case.widths))
    seg = case.seg and types.SimpleNamespace(k_score=case.seg, mlp=_blocks(case.widths[-1], (512, 256, 256, 128)))
    return module, seg or None


@functools.lru_cache(maxsize=None)
def _seg(Cd, k_score):
    from regnet_for_3d_grasping_amd.pointnet2 import PointNet2Seg
    return PointNet2Seg(input_chann=3 + Cd, k_score=k_score).eval()


def fp_module(case):
    """The real (module, seg or None); None where no PointNet2Seg has such a last block (its channels are the reference's)."""
    from regnet_for_3d_grasping_amd.pn2_utils.modules import PointnetFPModule
    if not case.seg:
        return PointnetFPModule(case.Cs + case.Cd, case.widths, 3).eval(), None
    if (case.Cs, case.widths) != (512, (256, 256, 256)):
        return None
    seg = _seg(case.Cd, case.seg)
    return seg.fp_modules[-1], seg


@contextlib.contextmanager
def switched(case):
    """fused.py under the row's switches and mode, restored afterwards."""
    import torch

    from regnet_for_3d_grasping_amd import fused
    assert set(case.switches) <= set(SWITCHES), case.switches
    saved = {k: getattr(fused, k) for k in case.switches}
    try:
        for k, v in case.switches.items():
            setattr(fused, k, v)
        with torch.set_grad_enabled(getattr(case, "mode", "eval") == "grad"):
            yield fused
    finally:
        for k, v in saved.items():
            setattr(fused, k, v)


def sa_launches(route, prepared=True):
    """Calls of fused.TIMED_OPS' wrappers that the feature stage of a set-abstraction block makes on ``route``, as a dict name ->
    count.  ``prepared``: the geometry stage made the route's V (its own mlp_layer call is then not the feature stage's)."""
    calls = {{"chain3": "sa_chain3", "premul_chain256": "sa_premul_chain", "premul_chain512": "sa3_premul_chain",
              "layer12": "sa_layer12", "premul_layer": "sa_premul_layer", "layer1": "sa_layer1"}[route.features]: 1}
    plain = route.tail + (route.features.startswith("premul") and 2 - bool(prepared))     # U, and V where nobody made it
    if plain:
        calls["mlp_layer"] = plain
    return calls


def fp_launches(route, layers):
    """... of a feature-propagation block of ``layers`` MLP layers (behind a head route: with the head)."""
    head = route.features.startswith("head")
    calls = {"head_interp": {"fp_head_chain_interp": 1}, "head_chain": {"fp_head_chain": 1}}.get(route.features, {})
    plain = (layers if route.features == "concat" else 1 + (route.skip == "gemm") + (0 if head else layers - 1))
    return dict(calls, mlp_layer=plain)
