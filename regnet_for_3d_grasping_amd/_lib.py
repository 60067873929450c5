"""ctypes loader for ``csrc/libregnet_hip.so`` (the C ABI declared in include/regnet_hip.h).

The header is the only declaration of an entry point: its prototypes are parsed at import into the ctypes signatures
(``parse_header``), and ``call`` is the one way to launch (device, stream, status).

Fails loudly: a missing library raises ImportError at import time and a non-zero status from
any entry point raises RuntimeError (the reference's TORCH_CHECK / THCudaCheck convention,
e.g. csrc/sampling_kernel.cu:134-137,167).
"""
import ctypes
import os
import re

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("REGNET_HIP_LIB") or os.path.join(_HERE, "csrc", "libregnet_hip.so")   # override: A/B builds only

HEADER_PATH = os.path.join(_HERE, "..", "include", "regnet_hip.h")

_CTYPES = {"int": ctypes.c_int, "int64_t": ctypes.c_int64, "uint64_t": ctypes.c_uint64, "float": ctypes.c_float,
           "double": ctypes.c_double}
_PROTOTYPE = re.compile(r"([^;{}()]*?)\b(regnet_\w+)\s*\(([^()]*)\)\s*;")


def parse_header(text):
    """The prototypes ``<ret> regnet_<name>(<params>);`` of a C header -> (SIGNATURES, PARAMS): name -> (restype, argtypes)
    and name -> parameter names.  Any pointer parameter is a ``c_void_p``, a ``const char*`` return a ``c_char_p``, scalars
    go through ``_CTYPES``; anything else raises ImportError naming the prototype -- the binding never guesses a type."""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
    text = re.sub(r"^[ \t]*#.*$", " ", text, flags=re.M)
    signatures, params = {}, {}
    for ret, name, plist in _PROTOTYPE.findall(text):
        ret = " ".join(ret.split()).replace(" *", "*")
        if ret == "const char*":
            restype = ctypes.c_char_p
        elif ret in _CTYPES:
            restype = _CTYPES[ret]
        else:
            raise ImportError("%s: return type %r has no ctypes mapping" % (name, ret))
        argtypes, names = [], []
        plist = plist.strip()
        for param in (plist.split(",") if plist != "void" else []):
            m = re.fullmatch(r"(.*?)(\w+)", " ".join(param.split()))
            ctype = m and (m.group(1).replace("const ", "").strip())
            if not ctype or not ("*" in ctype or ctype in _CTYPES):
                raise ImportError("%s: parameter %r has no ctypes mapping" % (name, param.strip()))
            argtypes.append(ctypes.c_void_p if "*" in ctype else _CTYPES[ctype])
            names.append(m.group(2))
        signatures[name], params[name] = (restype, argtypes), names
    if len(signatures) != len(set(re.findall(r"\b(regnet_\w+)\s*\(", text))):
        raise ImportError("a regnet_* declaration in the header is not a prototype this parser reads")
    if not signatures:
        raise ImportError("no regnet_* prototype found in the header")
    return signatures, params


# name -> (restype, argtypes) and name -> parameter names: include/regnet_hip.h is the only declaration of an entry point.
with open(HEADER_PATH) as _f:
    SIGNATURES, PARAMS = parse_header(_f.read())
# the launching entry points: their last parameter is the hipStream_t (the others are size, support and host-side queries)
HAS_STREAM = {name: names[-1:] == ["stream"] for name, names in PARAMS.items()}


def _load():
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            "libregnet_hip.so is not built (%s). Run `python -c 'import __graft_entry__ as g; g.build()'` "
            "or `python regnet_for_3d_grasping_amd/csrc/build.py`; there is no CPU fallback." % LIB_PATH)
    lib = ctypes.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)  # AttributeError here == header/library mismatch: fail loudly
        fn.restype = res
        fn.argtypes = args
    return lib


lib = _load()


def check(status, what):
    """Raise RuntimeError for a non-zero status code of entry point ``what``."""
    if status != 0:
        msg = lib.regnet_strerror(int(status)).decode()
        raise RuntimeError("%s failed: %s (code %d)" % (what, msg, status))


def call(name, anchor, *args, stream=None, tolerate=0):
    """Call entry point ``name`` for the GPU tensor ``anchor`` and return its value.  A launching entry point (last parameter
    ``stream``) runs with the anchor's device current -- a context is entered only when it is not already -- on ``stream`` (a
    raw handle; default: torch's current stream of that device), appended to ``args``; a non-zero status raises RuntimeError,
    except ``tolerate`` (a status on which the caller itself falls back).  An entry point without a stream parameter is
    called with ``args`` as they are."""
    fn = getattr(lib, name)
    if not HAS_STREAM[name]:
        return fn(*args)
    device = anchor.device
    if stream is None:
        stream = torch.cuda.current_stream(device).cuda_stream
    if device.index != torch.cuda.current_device():
        with torch.cuda.device(device):
            status = fn(*args, stream)
    else:
        status = fn(*args, stream)
    if status != 0 and status != tolerate:
        check(status, name)
    return status
