"""What the modules of the frame front end share (``ingest``, ``depth_frame``, ``fusion``, ``registration``, ``table_plane``, ``grasp_select``,
``segment``, ``detect``): host <-> device plumbing, argument checks, the one frame-size limit and the parameter classes'
``coerce``.  Host code only; torch is imported where it is needed, as in its neighbours.
"""
import contextlib

import numpy as np

MAX_FRAME_POINTS = 1 << 21          # rows of a frame, pixels of a depth image, voxels of a merge: larger is REGNET_ERR_UNSUPPORTED


def to_host(a):
    """A tensor (any device) or anything array-like -> a numpy array."""
    return a.detach().cpu().numpy() if hasattr(a, "detach") else np.asarray(a)


def to_device(a, device):
    """A host array or tensor -> a contiguous tensor on the GPU: host data goes up once through ``host_io``, as it is; a device
    tensor is used where it is."""
    import torch
    if isinstance(a, torch.Tensor) and a.is_cuda:
        return a.contiguous()
    from . import host_io
    return host_io.upload(a.contiguous() if isinstance(a, torch.Tensor) else np.ascontiguousarray(a), device).contiguous()


def matrix4(pose, what, finite=False):
    """``pose`` (array or tensor) -> (4, 4) float64 array; another shape (with ``finite``: or a NaN / infinite entry) is a
    ValueError saying ``what`` must be."""
    T = np.asarray(to_host(pose), dtype=np.float64)
    if T.shape != (4, 4) or (finite and not np.isfinite(T).all()):
        raise ValueError(what)
    return T


def require_cuda(name, t, dtype=None, cols=None, at_least=False, error=None):
    """``t`` must be a CUDA tensor (else RuntimeError) of shape (n, cols) -- (n, >= cols) with ``at_least``, (n) when ``cols``
    is None -- (else ValueError) and of ``dtype``, one or a tuple of them, None for any (else TypeError); ``error`` replaces the
    last two types.  -> ``t``, as it is: nothing is launched."""
    import torch
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise RuntimeError("%s must be a CUDA tensor (no CPU path)" % name)
    if cols is None:
        shape_ok = t.dim() == 1
    else:
        shape_ok = t.dim() == 2 and (t.shape[1] >= cols if at_least else t.shape[1] == cols)
    dtypes = dtype if isinstance(dtype, tuple) else (dtype,)
    if not shape_ok or (dtype is not None and t.dtype not in dtypes):        # (the message is put together only here)
        shape = "(n)" if cols is None else "(n, %s%d)" % (">=" if at_least else "", cols)
        if not shape_ok:
            raise (error or ValueError)("%s must be %s" % (name, shape))
        raise (error or TypeError)("%s must be %s %s" % (name, " or ".join(str(d).replace("torch.", "") for d in dtypes), shape))
    return t


def check_step(word, step):
    """A parameter class' ``step``, the distance between two samples of the hand: None, or positive and finite as a float32 too;
    else a ValueError that opens with ``word``."""
    if step is not None:
        with np.errstate(over="ignore", under="ignore"):
            step32 = np.float32(step)
        if not (float(step) > 0.0 and step32 > 0.0 and np.isfinite(step32)):
            raise ValueError("%s: step must be None or positive and finite in float32" % word)


def stream_scope(stream):
    """The context in which work is launched on ``stream`` (None: the current stream, nothing to enter)."""
    if stream is None:
        return contextlib.nullcontext()
    import torch
    return torch.cuda.stream(stream)


def record_streams(stream, *tensors):
    """Inputs read on ``stream`` (None: nothing to do) are kept alive for it; None entries are skipped."""
    if stream is not None:
        for t in tensors:
            if t is not None:
                t.record_stream(stream)


class ParamsBase:
    """``coerce`` of the front end's parameter dataclasses: an instance -> itself, a dict -> ``cls(**dict)``, None -> None, or
    the defaults where the class says ``NONE_IS_DEFAULT``; anything else is a TypeError naming ``WORD``, the detector's keyword."""
    WORD = "params"
    NONE_IS_DEFAULT = False

    @classmethod
    def coerce(cls, value):
        if value is None:
            return cls() if cls.NONE_IS_DEFAULT else None
        if isinstance(value, cls):
            return value
        if isinstance(value, dict):
            return cls(**value)
        raise TypeError("%s must be None, a dict or a %s" % (cls.WORD, cls.__name__))
