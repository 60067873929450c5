"""The case table of the training 1x1 convolutions (regnet_for_3d_grasping_amd/conv1x1_train.py): which kernels a layer of a
given shape runs on under given module switches.  Every expectation is written by hand from the rules in ``route``'s
documentation ("One route per layer"), never computed by calling it; tests/test_conv1x1_route_cpu.py holds ``route``
against the table and tests/test_gpu_conv1x1_route.py holds the launches of a real forward + backward against it.

A row is ``Case(shape, kind, switches, expect, otherwise)``:
  shape      (B, Co, Ci, L) of the convolution
  kind       "plain": ``conv1x1(conv, x, stats=True)``; "pending": the second convolution of conv -> bn -> relu -> conv, which
             consumes the first BatchNorm as a bn_train.Pending where it can
  switches   overrides of the module's upper-case switches; "deterministic": torch.use_deterministic_algorithms;
             "aligned": False -- the input does not start on 16 bytes
  expect     (fwd, pad, stats, dgrad, wgrad) with a training BatchNorm behind the layer, or None for a pending row whose
             convolution cannot consume the Pending
  otherwise  for such a row: the plain route the stack then takes for that convolution
The limits in the comments are those of csrc/tgemm.hip: channel counts multiples of 16 and >= 32, L a multiple of 4 and >= 64
(weight gradient: of 16); statistics up to 256 output channels (and 256 input channels of a pending operand); a pending operand
up to 512 channels and L a multiple of 16.
"""
import collections
import contextlib

Case = collections.namedtuple("Case", "shape kind switches expect otherwise")

FIELDS = ("fwd", "pad", "stats", "dgrad", "wgrad")
VALUES = {"fwd": {"stream", "tile", "split", "smallci", "bmm"}, "pad": {False, True}, "stats": {False, True},
          "dgrad": {"stream", "tile", "split", "bmm"}, "wgrad": {"tgemm", "smallci", "bmm"}}
SWITCHES = ("NATIVE", "STREAM", "PAD_CHANNELS", "FUSE_STATS", "DEFER_BN", "SPLIT_PRODUCTS")

NATIVE = ("stream", 0, True, "stream", "tgemm")            # the default kernels, statistics with the output
NO_STATS = ("stream", 0, False, "stream", "tgemm")
LIBRARY = ("bmm", 0, False, "bmm", "bmm")
SMALL = ("smallci", 0, True, "bmm", "smallci")


def _plain(shape, expect, **switches):
    return Case(shape, "plain", switches, expect, None)


def _pending(shape, expect, otherwise=None, **switches):
    return Case(shape, "pending", switches, expect, otherwise)


CASES = [
    _plain((2, 64, 64, 256), NATIVE),
    _pending((2, 64, 64, 256), NATIVE),
    # ---- input channels: 8 | 9 store stream / padded to 32; 31 | 32 | 33 padded / native / padded to 48; 259, 515 ---------
    _plain((2, 64, 8, 256), SMALL),
    _plain((2, 64, 9, 256), ("stream", 32, True, "stream", "tgemm")),
    _plain((2, 64, 31, 256), ("stream", 32, True, "stream", "tgemm")),
    _plain((2, 64, 32, 256), NATIVE),
    _plain((2, 64, 33, 256), ("stream", 48, True, "stream", "tgemm")),
    _plain((2, 64, 259, 256), ("stream", 272, True, "stream", "tgemm")),
    _plain((1, 64, 515, 256), ("stream", 528, True, "stream", "tgemm")),
    # ---- output channels: 16 | 32 (at least 32), 40 (no multiple of 16), 256 | 272 (statistics up to 256) -------------------
    _plain((2, 16, 64, 256), LIBRARY),
    _plain((2, 32, 64, 256), NATIVE),
    _plain((2, 40, 64, 256), LIBRARY),
    _plain((2, 256, 64, 256), NATIVE),
    _plain((2, 272, 64, 256), NO_STATS),
    # ---- points: 60 | 64 (at least 64), 77 (no multiple of 4), 1000 (of 4, not of 16: no native weight gradient), 4160 ------
    _plain((2, 64, 64, 60), LIBRARY),
    _plain((2, 64, 64, 64), NATIVE),
    _plain((2, 64, 64, 77), LIBRARY),
    _plain((2, 64, 64, 1000), ("stream", 0, True, "stream", "bmm")),
    _plain((2, 64, 64, 4160), NATIVE),
    _plain((2, 64, 259, 1000), LIBRARY),                   # padding only where the weight gradient stays native too
    _plain((2, 64, 6, 1000), SMALL),                       # the store streams ask for a multiple of 4 only
    _plain((2, 64, 6, 78), LIBRARY),
    # ---- one switch each ------------------------------------------------------------------------------------------------------
    _plain((2, 64, 64, 256), LIBRARY, NATIVE=False),
    _plain((2, 64, 6, 256), LIBRARY, NATIVE=False),
    _plain((2, 64, 64, 256), ("tile", 0, False, "tile", "tgemm"), STREAM=False),      # statistics: the persistent kernel only
    _plain((2, 64, 259, 256), ("tile", 272, False, "tile", "tgemm"), STREAM=False),
    _plain((2, 64, 6, 256), SMALL, STREAM=False),
    _plain((2, 64, 259, 256), LIBRARY, PAD_CHANNELS=False),
    _plain((2, 64, 64, 256), NO_STATS, FUSE_STATS=False),
    _plain((2, 64, 6, 256), ("smallci", 0, False, "bmm", "smallci"), FUSE_STATS=False),
    _plain((2, 64, 64, 256), NATIVE, DEFER_BN=False),      # (a plain convolution does not read it)
    _plain((2, 64, 64, 256), ("split", 0, False, "split", "tgemm"), SPLIT_PRODUCTS=True),
    _plain((2, 64, 259, 256), ("split", 272, False, "split", "tgemm"), SPLIT_PRODUCTS=True),
    _plain((2, 64, 64, 1000), ("split", 0, False, "split", "bmm"), SPLIT_PRODUCTS=True),
    _plain((2, 16, 48, 36), LIBRARY, SPLIT_PRODUCTS=True),  # the experiment replaces native contractions only
    _plain((2, 64, 6, 256), SMALL, SPLIT_PRODUCTS=True),
    _plain((2, 64, 64, 256), NO_STATS, deterministic=True),  # fp64 atomics: bn_train's deterministic pass takes the statistics
    _plain((2, 64, 6, 256), ("smallci", 0, False, "bmm", "smallci"), deterministic=True),
    _plain((2, 64, 6, 256), LIBRARY, aligned=False),
    _plain((2, 64, 8, 64), LIBRARY, aligned=False),
    # ---- consuming a pending BatchNorm: 512 | 528 operand channels, statistics up to 256 | 272 of them ----------------------
    _pending((2, 64, 256, 256), NATIVE),
    _pending((2, 64, 272, 256), NO_STATS),
    _pending((2, 64, 512, 256), NO_STATS),
    _pending((1, 64, 528, 256), None, NATIVE),
    _pending((2, 256, 64, 256), NATIVE),
    _pending((2, 272, 64, 256), NO_STATS),
    _pending((2, 64, 64, 256), None, NATIVE, DEFER_BN=False),
    _pending((2, 64, 64, 256), None, ("tile", 0, False, "tile", "tgemm"), STREAM=False),
    _pending((2, 64, 64, 256), None, LIBRARY, NATIVE=False),
    _pending((2, 64, 64, 256), NO_STATS, FUSE_STATS=False),
    _pending((2, 64, 64, 256), NO_STATS, deterministic=True),
    _pending((2, 64, 64, 256), ("split", 0, False, "split", "tgemm"), SPLIT_PRODUCTS=True),
    # ---- test_gemm_conv1x1_matches_torch_convolution (tests/test_gpu_train.py) ------------------------------------------------
    _plain((2, 32, 6, 2560), SMALL),
    _plain((3, 64, 259, 4096), ("stream", 272, True, "stream", "tgemm")),
    _plain((1, 128, 128, 131072), NATIVE),
    _plain((2, 3, 5, 77), LIBRARY),
    _plain((2, 128, 256, 4160), NATIVE),
    _plain((3, 48, 64, 2064), NATIVE),
    _plain((1, 1024, 512, 1024), NO_STATS),
    _plain((2, 512, 1024, 192), NO_STATS),
    _plain((4, 256, 128, 8192), NATIVE),
    # ---- test_statistics_left_by_the_convolution (tests/test_gpu_bn_train.py) --------------------------------------------------
    _plain((2, 128, 128, 19200), NATIVE),
    _pending((2, 256, 128, 19200), NATIVE),
    _pending((3, 160, 64, 4112), NATIVE),
    _plain((1, 64, 256, 1000), ("stream", 0, True, "stream", "bmm")),
    _plain((8, 128, 32, 131072), NATIVE),
    # ---- test_deferred_batchnorm_between_convolutions (tests/test_gpu_bn_train.py): every convolution of every stack ---------
    _plain((2, 64, 64, 19200), NATIVE), _pending((2, 128, 64, 19200), NATIVE), _pending((2, 128, 128, 19200), NATIVE),
    _plain((3, 128, 128, 4112), NATIVE), _pending((3, 64, 128, 4112), NATIVE), _pending((3, 256, 64, 4112), NATIVE),
    _plain((8, 64, 32, 131072), NATIVE), _pending((8, 64, 64, 131072), NATIVE),
    _plain((1, 512, 256, 640), NO_STATS), _pending((1, 256, 512, 640), NO_STATS), _pending((1, 128, 256, 640), NATIVE),
    _plain((2, 64, 6, 8192), SMALL), _pending((2, 64, 64, 8192), NATIVE), _pending((2, 128, 64, 8192), NATIVE),
    _plain((2, 1024, 512, 1024), NO_STATS), _pending((2, 256, 1024, 1024), None, NATIVE), _pending((2, 128, 256, 1024), NATIVE),
    _plain((2, 128, 128, 1000), ("stream", 0, True, "stream", "bmm")),
    _pending((2, 128, 128, 1000), None, ("stream", 0, True, "stream", "bmm")),
]


def case_id(case):
    return "%s-%s%s" % (case.kind, "x".join(map(str, case.shape)), "".join("-%s=%d" % kv for kv in sorted(case.switches.items())))


@contextlib.contextmanager
def switched(switches):
    """The module under ``switches`` (see the table's header; "aligned" is the caller's to act on), restored afterwards."""
    import torch

    from regnet_for_3d_grasping_amd import conv1x1_train
    module = {k: v for k, v in switches.items() if k in SWITCHES}
    assert set(switches) <= set(SWITCHES) | {"deterministic", "aligned"}, switches
    saved = {k: getattr(conv1x1_train, k) for k in module}
    deterministic = torch.are_deterministic_algorithms_enabled()
    try:
        for k, v in module.items():
            setattr(conv1x1_train, k, v)
        torch.use_deterministic_algorithms(bool(switches.get("deterministic", deterministic)))
        yield conv1x1_train
    finally:
        torch.use_deterministic_algorithms(deterministic)
        for k, v in saved.items():
            setattr(conv1x1_train, k, v)


def launches(case):
    """The launching ``regnet_conv1x1_*`` entry points a forward + backward of the row's convolution calls, in order; a bmm
    contraction calls none."""
    route = case.expect if case.expect is not None else case.otherwise
    fwd, _, stats, dgrad, wgrad = route
    affine = case.kind == "pending" and case.expect is not None
    if fwd == "smallci":
        first = "fwd_smallci_stats_f32" if stats else "fwd_smallci_f32"
    elif stats:
        first = "fwd_stats_stream_f32"
    else:
        first = {"stream": "fwd_bnrelu_stream_f32" if affine else "fwd_stream_f32", "tile": "fwd_f32", "split": "split_f32",
                 "bmm": None}[fwd]
    second = {"stream": "dgrad_stream_f32", "tile": "dgrad_f32", "split": "split_f32", "bmm": None}[dgrad]
    third = {"tgemm": "wgrad_bnrelu_f32" if affine else "wgrad_f32", "smallci": "wgrad_smallci_f32", "bmm": None}[wgrad]
    return ["regnet_conv1x1_" + name for name in (first, second, third) if name]
