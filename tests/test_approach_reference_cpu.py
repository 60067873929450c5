"""Approach analysis without a GPU: the C ABI's new entry point (exported, declared, argument checks before any launch), the
numpy restatement of the contract (tests/approach_reference.py) against answers derived by hand and against the collision
oracle's counts, the parameter class and the CLI flags."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

from . import approach_reference as ref

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "regnet_grasp_approach_f32"


def test_new_symbol_is_exported_bound_declared_and_built_without_contraction():
    from regnet_for_3d_grasping_amd import _lib
    from regnet_for_3d_grasping_amd.csrc import build
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "regnet_hip.h")).read(), flags=re.S)
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), NAME)
    assert re.search(r"\b%s\s*\(" % NAME, header)
    vp, i64, f = ctypes.c_void_p, ctypes.c_int64, ctypes.c_float
    assert _lib.SIGNATURES[NAME] == (ctypes.c_int, [vp, i64, i64, vp, i64, i64, i64, vp, i64, f, f, vp, f, f, f, f, f, f, f, vp, vp,
                                                   vp])
    assert _lib.HAS_STREAM[NAME]
    assert dict(build.SOURCES)["approach.hip"] == ["-ffp-contract=off"]
    assert _lib.lib.regnet_abi_version() == 2


def _raw(points=1, N=5, T=1, B=2, standoff=0.1, counts=1, values=1, normals=None):
    from regnet_for_3d_grasping_amd import _lib
    return _lib.lib.regnet_grasp_approach_f32(points, 3, 1, normals, 3, 1, N, T, B, -0.06, 0.06, None, 0.005, 0.05, 0.04, -0.0,
                                              standoff, 0.005, 0.5, counts, values, None)


def test_argument_checks_without_gpu():
    # validation happens before any launch, so these are safe without a device (the non-NULL pointers are never followed)
    assert _raw(N=-1) == -1 and _raw(B=-1) == -1                                     # REGNET_ERR_SHAPE
    assert _raw(N=1 << 31) == -3 and _raw(B=1 << 31) == -3                           # REGNET_ERR_UNSUPPORTED
    for bad in (-0.01, float("nan"), float("inf"), float("-inf")):
        assert _raw(standoff=bad) == -3, bad
        assert _raw(standoff=bad, B=0) == -3, bad                                    # ... even with nothing to do
    assert _raw(N=-1, standoff=-1.0) == -1                                           # the shape error comes first
    assert _raw(B=0, points=None, T=None, counts=None, values=None) == 0             # empty: no pointer touched, no launch
    assert _raw(T=None) == -2 and _raw(counts=None) == -2 and _raw(values=None) == -2 and _raw(points=None) == -2   # ..._NULL
    assert _raw(N=(1 << 31) - 1, B=(1 << 31) - 1, T=None) == -2                      # the limits themselves are supported


@pytest.mark.parametrize("case", ref.known_cases(), ids=lambda c: c[0])
def test_reference_gives_the_hand_derived_answers(case):
    _, inputs, counts, values = case
    got_counts, got_values = ref.approach_ref(inputs["points"], inputs["normals"], inputs["T"], inputs["box"], inputs["standoff"],
                                              inputs["contact_depth"], inputs["cos_friction"])
    assert got_counts.dtype == np.int32 and got_values.dtype == np.float32
    assert np.array_equal(got_counts, counts), (got_counts, counts)
    assert got_values.tobytes() == values.tobytes(), (got_values, values)
    if inputs["normals"] is not None:                    # without normals: the same pass 1, pass 2's counts 0
        c0, v0 = ref.approach_ref(inputs["points"], None, inputs["T"], inputs["box"], inputs["standoff"], inputs["contact_depth"],
                                  inputs["cos_friction"])
        assert np.array_equal(c0[:, :3], counts[:, :3]) and not c0[:, 3:].any() and v0.tobytes() == values.tobytes()


def test_known_cases_cover_every_output():
    cases = ref.known_cases()
    counts = np.concatenate([c[2] for c in cases])
    assert (counts[:, :7].max(0) > 0).all() and not counts[:, 7].any()
    values = np.concatenate([c[3] for c in cases])
    assert np.isinf(values[:, 0]).any() and np.isfinite(values[:, 0]).any()
    assert len({float(v) for v in values[:, 2]}) >= 3    # the standoff, a retreat in between and 0


@pytest.mark.parametrize("per_grasp_depth", [False, True])
def test_region_and_hand_counts_are_the_collision_oracles(per_grasp_depth):
    from oracle import collision_oracle as oracle
    rng = np.random.default_rng(11)
    grasp, points, normals = ref.random_case(3, 3000, 24)
    frame, center = oracle.grasp_frames(torch.from_numpy(grasp))
    T = oracle.global_to_local(frame, center).numpy()
    depth = rng.uniform(0.02, 0.08, len(grasp)).astype(np.float32) if per_grasp_depth else 0.06
    want = oracle.collision_counts(points, T, depth, 0.08)
    counts, values = ref.approach_ref(points, normals, T, ref.gripper_box(depth, 0.08), 0.1, ref.NEIGHBOR_DEPTH,
                                      ref.cos_friction(30.0))
    assert want[:, 3].max() > 16 and (want[:, 1] + want[:, 2]).max() > 0            # not a comparison of zeros
    assert np.array_equal(counts[:, 0], want[:, 3])
    assert np.array_equal(counts[:, 2], want[:, 1] + want[:, 2])
    # the cloud exercises everything else as well: blockers in between, both bands, normals inside and outside the cone
    assert ((values[:, 2] > 0) & (values[:, 2] < np.float32(0.1))).any() and (counts[:, 1] > 0).any()
    assert (counts[:, 3] > counts[:, 4]).any() and (counts[:, 4] > 0).any() and (counts[:, 5] > counts[:, 6]).any()
    # the y extent is the one the oracle's antipodal score is built on: its score is finite exactly where both bands have points
    score = oracle.antipodal_scores(points, normals, T, depth, 0.08)
    assert np.array_equal(np.isfinite(score), (counts[:, 3] > 0) & (counts[:, 5] > 0))
    # the gripper's box is eval_collision's
    from regnet_for_3d_grasping_amd import eval_collision
    box, _ = eval_collision._box_args(0.06, 0.08, 1, "cpu")
    mine = ref.gripper_box(0.06, 0.08)
    assert [np.float32(v) for v in box[:2] + box[3:]] == [mine[0], mine[1]] + list(mine[2:])
    assert ref.NEIGHBOR_DEPTH == eval_collision.NEIGHBOR_DEPTH


def test_derived_tensors_of_the_known_cases():
    case = {c[0]: c for c in ref.known_cases()}
    frame = np.eye(3, dtype=np.float32)[None]
    center = np.array([[1.0, 2.0, 3.0]], dtype=np.float32)
    _, _, counts, values = case["contact_bands"]
    d = ref.derived_ref(counts, values, frame, center, pad=0.0625, half_space=0.75)
    assert d["grasp_width"].tolist() == [1.0] and d["grasp_offset"].tolist() == [0.0] and d["grasp_opening"].tolist() == [1.125]
    assert d["grasp_contact"].tolist() == [0.5] and d["grasp_clearance"].tolist() == [1.0]
    assert d["grasp_pregrasp"].tolist() == [[0.0, 2.0, 3.0]]
    assert ref.derived_ref(counts, values, frame, center, pad=0.5, half_space=0.75)["grasp_opening"].tolist() == [1.5]   # capped
    _, _, counts, values = case["wall_behind"]           # an empty region: zero width, offset and contact
    d = ref.derived_ref(counts, values, frame, center, pad=0.0625, half_space=0.75)
    assert d["grasp_width"].tolist() == [0.0] and d["grasp_offset"].tolist() == [0.0] and d["grasp_contact"].tolist() == [0.0]
    assert d["grasp_opening"].tolist() == [0.125] and d["grasp_pregrasp"].tolist() == [[0.75, 2.0, 3.0]]
    assert ref.passes_ref(d).tolist() == [True] and ref.passes_ref(d, min_clearance=0.25).tolist() == [True]
    assert ref.passes_ref(d, min_clearance=0.26).tolist() == [False] and ref.passes_ref(d, min_contact=0.1).tolist() == [False]
    for dtype_check in d.values():
        assert dtype_check.dtype == np.float32


def test_cos_friction_is_rounded_once():
    from regnet_for_3d_grasping_amd import approach
    for deg in (0.0, 10.0, 30.0, 45.0, 60.0, 89.9, 90.0):
        got = approach.cos_friction(deg)
        assert isinstance(got, float) and float(np.float32(got)) == got
        assert np.float32(got) == np.float32(math.cos(math.radians(deg))) == ref.cos_friction(deg)
    # not the float32 cosine of a float32 angle: the two differ somewhere on a fine grid of angles
    grid = np.arange(1, 9000) / 100.0
    once = np.array([approach.cos_friction(a) for a in grid], dtype=np.float32)
    assert (once != np.cos(np.radians(grid.astype(np.float32)))).any()
    assert approach.cos_friction(None) == 0.0


def test_params():
    from regnet_for_3d_grasping_amd import approach, eval_collision, grasp_select
    P = approach.ApproachParams
    p = P()
    assert (p.source, p.standoff, p.contact_depth, p.friction_deg, p.normal_radius, p.normal_max_nn, p.pad, p.min_clearance,
            p.min_contact) == (None, 0.10, eval_collision.NEIGHBOR_DEPTH, None, eval_collision.NORMAL_RADIUS,
                               eval_collision.NORMAL_MAX_NN, 0.005, None, None)
    assert P.WORD == "approach" and P.coerce(None) is None and P.coerce(p) is p
    q = P.coerce({"standoff": 0.05, "friction_deg": 20.0, "min_clearance": 0.03})
    assert type(q) is P and q == P(standoff=0.05, friction_deg=20.0, min_clearance=0.03) and q.filters() and not p.filters()
    assert P(min_contact=0.5).filters()
    for bad in ("x", 3, [1]):
        with pytest.raises(TypeError, match=r"^approach must be None, a dict or a ApproachParams$"):
            P.coerce(bad)
    with pytest.raises(TypeError):
        P.coerce({"no_such_field": 1})
    for source in grasp_select.SOURCES:
        assert P(source=source).source == source
    for bad in ({"source": "grasp_stage4"}, {"source": "points"}, {"standoff": -0.01}, {"standoff": float("inf")},
                {"standoff": float("nan")}, {"friction_deg": 91.0}, {"friction_deg": -1.0}, {"pad": -0.001}):
        with pytest.raises(ValueError, match="^approach: "):
            P(**bad)
    with pytest.raises(RuntimeError, match="CUDA tensor"):           # GPU only
        approach.analyse(torch.zeros((4, 3)), torch.zeros((1, 8)), 0.06, 0.08)


CLI_REQUIRED = ["--folder", "f", "--load-score-path", "s", "--load-region-path", "r"]


def test_cli_flags_turn_the_stage_on_and_off():
    from regnet_for_3d_grasping_amd import approach, detect
    assert detect.APPROACH_KEYS == ("grasp_clearance", "grasp_width", "grasp_offset", "grasp_opening", "grasp_contact",
                                    "grasp_pregrasp")
    parser = detect.build_parser()
    assert detect.approach_from_args(parser.parse_args(CLI_REQUIRED)) is None
    assert detect.approach_from_args(parser.parse_args(CLI_REQUIRED + ["--top-k", "5", "--segment"])) is None
    assert detect.approach_from_args(parser.parse_args(CLI_REQUIRED + ["--approach"])) == {}
    each = (("--approach-standoff", "0.05", {"standoff": 0.05}), ("--approach-from", "grasp_stage2", {"source": "grasp_stage2"}),
            ("--friction-angle", "25", {"friction_deg": 25.0}), ("--min-clearance", "0.04", {"min_clearance": 0.04}),
            ("--min-contact", "0.5", {"min_contact": 0.5}))
    everything, flags = {}, []
    for flag, value, want in each:                       # any of the five turns the stage on
        got = detect.approach_from_args(parser.parse_args(CLI_REQUIRED + [flag, value]))
        assert got == want and approach.ApproachParams.coerce(got) == approach.ApproachParams(**want)
        everything.update(want)
        flags += [flag, value]
    assert detect.approach_from_args(parser.parse_args(CLI_REQUIRED + ["--approach"] + flags)) == everything
    with pytest.raises(SystemExit):
        parser.parse_args(CLI_REQUIRED + ["--approach-from", "points"])
    helps = {a.dest: a.help for a in parser._actions}
    assert "(0.1 m)" in helps["approach_standoff"]
    parser.format_help()
    # the other groups' dicts do not see the new flags
    full = parser.parse_args(CLI_REQUIRED + ["--approach"] + flags)
    assert detect.select_from_args(full) is None and detect.segment_from_args(full) is None


def test_detector_refuses_a_filter_on_a_set_the_selection_does_not_read():
    """Construction-time checks that need no GPU run: a CPU network is refused later, so they are made on the arguments."""
    from regnet_for_3d_grasping_amd import detect
    with pytest.raises(TypeError, match="^approach must be None"):
        detect.GraspDetector(None, None, approach="yes")
    with pytest.raises(ValueError, match="^approach: source"):
        detect.GraspDetector(None, None, approach={"source": "nope"})
    with pytest.raises(ValueError, match="^approach: min_clearance / min_contact filter the selection"):
        detect.GraspDetector(None, None, select={"source": "grasp_stage2"}, approach={"source": "grasp_stage3", "min_clearance": 0.05})
    with pytest.raises(ValueError, match="^approach: min_clearance / min_contact filter the selection"):
        detect.GraspDetector(None, None, segment={"source": "grasp_stage2", "top_k_per_object": 2}, approach={"min_contact": 0.5})
