"""Deterministic mode of the float32 training path.

The mode is on exactly when ``torch.are_deterministic_algorithms_enabled()`` is true: there is no switch of this package's
own.  Under it, every sum our kernels form in a training iteration is added in one fixed order (the sort plan and
segment sums of csrc/scatter.hip, which the float64 backwards share; csrc/det.hip; csrc/bn_train.hip ``_det`` entry
points), so two runs from the same state and seeds agree bit for bit.  With the mode off nothing changes: the default kernels run as before.

An op that has no deterministic kernel for a shape raises RuntimeError naming itself, as torch's own ops do; under
``torch.use_deterministic_algorithms(True, warn_only=True)`` it warns once per op and runs its default kernel.

The guarantee is per process, on one device, with one rank: the order of a gradient all-reduce over several ranks is
outside it.
"""
import warnings

import torch

REGNET_ERR_UNSUPPORTED = -3
_warned = set()


def enabled():
    return torch.are_deterministic_algorithms_enabled()


def unsupported(op, what=""):
    """``op`` has no deterministic kernel for this call: raise, or (warn_only) warn once and return so that the caller runs
    its default kernel."""
    msg = ("%s does not have a deterministic implementation%s, but you set 'torch.use_deterministic_algorithms(True)'"
           % (op, " for " + what if what else ""))
    if not torch.is_deterministic_algorithms_warn_only_enabled():
        raise RuntimeError(msg)
    if op not in _warned:
        _warned.add(op)
        warnings.warn(msg + "; running the default (non-deterministic) kernel", UserWarning, stacklevel=3)
