"""The fixed-order moments of the table plane without a GPU: the entry points are exported, declared and bound, their argument
checks return before any launch, and the workspace formula holds at the limits."""
import ctypes

import pytest

NEW_SYMBOLS = ("regnet_plane_moments_det_workspace_bytes", "regnet_plane_moments_det_f32", "regnet_plane_moments_det_f64")
MAX_M = 1 << 21


def test_symbols_and_workspace():
    from regnet_for_3d_grasping_amd import _lib
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert hasattr(raw, name) and name in _lib.SIGNATURES, name
    assert len(_lib.SIGNATURES["regnet_plane_moments_det_f32"][1]) == 6 and _lib.HAS_STREAM["regnet_plane_moments_det_f64"]
    ws = _lib.lib.regnet_plane_moments_det_workspace_bytes
    assert [ws(M) for M in (0, 1, 2048, 2049, 307200, MAX_M)] == [80, 80, 80, 160, 80 * 150, 80 * 1024]
    assert ws(-1) == -1 and ws(MAX_M + 1) == -1
    assert _lib.lib.regnet_abi_version() == 2


@pytest.mark.parametrize("name", NEW_SYMBOLS[1:])
def test_argument_checks_without_gpu(name):
    from regnet_for_3d_grasping_amd import _lib
    fn = getattr(_lib.lib, name)
    # validation happens before any launch, so these are safe without a device
    assert fn(1, -1, 1, 1, 1, None) == -1
    assert fn(1, MAX_M + 1, 1, 1, 1, None) == -3
    assert fn(None, 10, 1, 1, 1, None) == -2 and fn(1, 10, None, 1, 1, None) == -2
    assert fn(1, 10, 1, None, 1, None) == -2 and fn(1, MAX_M, 1, 1, None, None) == -2
