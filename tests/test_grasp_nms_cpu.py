"""Pose NMS + top-K without a GPU: the C ABI's new entry points (exported, declared, argument checks before any launch), the
numpy restatement of the contract (tests/nms_reference.py) against answers derived by hand, and the binding's CPU-tensor check."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from . import nms_reference as ref

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("regnet_grasp_nms_workspace_bytes", "regnet_grasp_nms_f32")
MAX_N = 32768


def test_new_symbols_are_exported_bound_and_declared():
    from regnet_for_3d_grasping_amd import _lib
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "regnet_hip.h")).read(), flags=re.S)
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert hasattr(raw, name), name
        assert name in _lib.SIGNATURES, name
        assert re.search(r"\b%s\s*\(" % name, header), name
    assert len(_lib.SIGNATURES["regnet_grasp_nms_f32"][1]) == 12
    assert _lib.lib.regnet_abi_version() == 2


def test_argument_checks_without_gpu():
    from regnet_for_3d_grasping_amd import _lib, grasp_select
    L = _lib.lib
    nms = L.regnet_grasp_nms_f32
    # validation happens before any launch, so these are safe without a device
    assert nms(None, None, None, -1, 0.001, 2.7, 1, 0, None, None, None, None) == -1       # n < 0
    assert nms(None, None, None, 0, 0.001, 2.7, 1, 0, None, None, None, None) == 0         # empty: no pointer touched
    assert nms(None, None, None, 5, 0.001, 2.7, 1, 0, None, None, None, None) == -2        # null pointers
    assert nms(1, 1, 1, 5, 0.001, 2.7, 1, 0, 1, 1, None, None) == -2                       # ... the workspace among them
    assert nms(None, None, None, MAX_N + 1, 0.001, 2.7, 1, 0, None, None, None, None) == -3
    assert nms(1, 1, 1, MAX_N + 1, 0.001, 2.7, 1, 0, 1, 1, 1, None) == -3
    assert nms(None, None, None, MAX_N, 0.001, 2.7, 1, 0, None, None, None, None) == -2    # the limit itself is supported
    ws = L.regnet_grasp_nms_workspace_bytes
    for n in (0, 1, 63, 64, 65, 128, 4000, 16000, MAX_N):
        nb = (n + 63) // 64
        assert ws(n) == nb * (nb + 1) // 2 * 64 * 8 == grasp_select.workspace_bytes(n), n
    assert ws(0) == 0 and ws(1) == 512 and ws(65) == 3 * 512
    assert ws(MAX_N) == 67239936                                                           # 64.1 MiB at the limit
    assert ws(-1) == -1 and ws(MAX_N + 1) == -1
    assert grasp_select.MAX_GRASPS == MAX_N


def test_thresholds_are_float32_values():
    from regnet_for_3d_grasping_amd import grasp_select
    for t, deg in ((0.03, 30.0), (ref.T_EXACT, 15.0), (0.1, 90.0), (1e-3, 0.0), (0.5, 180.0)):
        T2, C = grasp_select.thresholds(t, deg)
        rT2, rC = ref.thresholds(t, deg)
        assert np.float32(T2) == rT2 and float(np.float32(T2)) == T2
        assert np.float32(C) == rC and float(np.float32(C)) == C
    assert grasp_select.thresholds(ref.T_EXACT, 0.0) == (2.0 ** -10, 3.0)


@pytest.mark.parametrize("case", ref.known_cases(), ids=lambda c: c[0])
def test_reference_gives_the_hand_derived_answers(case):
    _, center, frame, score, kw, expected = case
    for fn in (ref.pose_nms_plain, ref.pose_nms_ref):
        keep, count = fn(center, frame, score, **kw)
        assert keep.dtype == np.int64 and keep.shape == (len(center),)
        assert count == len(expected) and keep[:count].tolist() == expected
        assert (keep[count:] == -1).all()


@pytest.mark.parametrize("seed,n,symmetric,top_k", [(1, 1, True, None), (2, 2, False, None), (3, 65, True, None),
                                                    (4, 130, False, None), (5, 300, True, None), (6, 300, False, 7),
                                                    (7, 200, True, 200)])
def test_array_walk_equals_the_plain_double_loop(seed, n, symmetric, top_k):
    center, frame, score = ref.clustered_poses(seed, n)
    score[::7] = score[0]                       # ties
    if n > 10:
        score[3], score[5] = np.nan, -0.0
    a = ref.pose_nms_plain(center, frame, score, 0.02, 20.0, top_k, symmetric)
    b = ref.pose_nms_ref(center, frame, score, 0.02, 20.0, top_k, symmetric)
    assert a[1] == b[1] and a[0].tolist() == b[0].tolist()
    if n >= 65 and top_k is None:
        assert 1 < a[1] < n                     # both suppressed and kept grasps


def test_rank_order():
    s = np.array([0.5, np.nan, 0.5, -0.0, 0.0, -np.inf, 2.0], dtype=np.float32)
    assert ref.rank_order(s).tolist() == [6, 0, 2, 3, 4, 1, 5]


def test_binding_rejects_cpu_tensors():
    from regnet_for_3d_grasping_amd import grasp_select
    g = torch.zeros(4, 8)
    for call in (lambda: grasp_select.pose_nms(g), lambda: grasp_select.pose_nms_device(g),
                 lambda: grasp_select.pose_nms(torch.zeros(0, 8)),
                 lambda: grasp_select.nms_ranked(torch.zeros(4, 3), torch.zeros(4, 3, 3), torch.zeros(4, dtype=torch.int64))):
        with pytest.raises(RuntimeError, match="CUDA tensor"):
            call()


def test_select_params():
    from regnet_for_3d_grasping_amd import detect, grasp_select
    assert grasp_select.SelectParams.coerce(None) is None
    p = grasp_select.SelectParams.coerce({"top_k": 5})
    assert (p.source, p.top_k, p.translation_thresh, p.rotation_thresh_deg, p.symmetric) == ("grasp_stage3", 5, 0.03, 30.0, True)
    assert grasp_select.SelectParams.coerce(p) is p
    with pytest.raises(ValueError):
        grasp_select.SelectParams(source="points")
    assert grasp_select.SOURCES == detect.RESULT_KEYS[3:]
    assert detect.SELECT_KEYS == ("grasp_selected", "grasp_selected_index")


def test_cli_flags_turn_selection_on():
    import argparse
    from regnet_for_3d_grasping_amd import detect
    ns = argparse.Namespace(top_k=None, nms_translation=None, nms_rotation=None, select_from=None)
    assert detect.select_from_args(ns) is None
    ns.top_k = 10
    assert detect.select_from_args(ns) == {"top_k": 10}
    ns = argparse.Namespace(top_k=None, nms_translation=0.02, nms_rotation=15.0, select_from="grasp_stage2")
    assert detect.select_from_args(ns) == {"translation_thresh": 0.02, "rotation_thresh_deg": 15.0, "source": "grasp_stage2"}


def test_unit_or_fallback_rows():
    """eval_collision._unit_or builds its fallback rows without a host upload (so grasp_frames can be captured): same values."""
    from regnet_for_3d_grasping_amd import eval_collision
    v = torch.tensor([[3.0, 0.0, 4.0], [0.0, 0.0, 0.0], [0.0, -2.0, 0.0]])
    out = eval_collision._unit_or(v, [0.0, 1.0, 0.0])
    assert out.dtype == torch.float32 and out.is_contiguous()
    assert torch.equal(out, torch.tensor([[0.6, 0.0, 0.8], [0.0, 1.0, 0.0], [0.0, -1.0, 0.0]]))
