"""``GraspDetector(approach=...)`` end to end on synthetic.make_batch's scene, where grasps survive the collision filter: the
record's ``APPROACH_KEYS`` against the numpy restatement (tests/approach_reference.py) run on the record's own points and source
set, a wall planted behind chosen grasps, the filtered selection, the unchanged default record and the CLI flags.  The fixture
pattern is the one of tests/test_gpu_detect_segment.py, copied."""
import contextlib
import io
import pickle

import numpy as np
import pytest
import torch

from . import approach_reference as ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SEED = 1234
SCENE_BOUNDS = (0.5, -0.5, 1.0, 0.5, -0.5)  # synthetic.make_batch's table with room to spare (tests/test_gpu_detect.py)
f32 = np.float32


def _region(net, g, pc, feat, gp):
    with contextlib.redirect_stdout(io.StringIO()), torch.no_grad():
        return net(g[3], g[5], g[2], g[4], g[0], g[1], pc, feat, gp, None, [])


def _scene_frame():
    """synthetic.make_batch(1000, 1)'s scene lifted into camera coordinates, colours on the 8-bit grid."""
    from regnet_for_3d_grasping_amd import ingest, synthetic
    scene = synthetic.make_batch(1000, 1, 25600)[0].numpy().astype(np.float64)
    Tinv = np.linalg.inv(ingest.table_frame_transform())
    return scene[:, :3] @ Tinv[:3, :3].T + Tinv[:3, 3], np.rint(scene[:, 3:6] * 255.0) / 255.0


@pytest.fixture(scope="module")
def parts():
    """Networks calibrated on the frame's own cropped cloud -> (score_net, region_net, frame, detector keywords)."""
    from regnet_for_3d_grasping_amd import detect, np_random, pipeline, synthetic
    from regnet_for_3d_grasping_amd.get_regiondataset import get_grasp_allobj
    xyz, rgb = _scene_frame()
    kw = {"bounds": SCENE_BOUNDS}
    score_net, region_net = pipeline.build_models(DEV)
    score_net.eval()
    region_net.eval()
    probe = detect.GraspDetector(score_net, region_net, **kw)
    np.random.seed(SEED)
    with np_random.deferred(), torch.no_grad():
        pc = probe.ingest((xyz, rgb)).pc.clone()
    synthetic.calibrate_score_head(score_net, pc)
    with torch.no_grad():
        feat, score, _ = score_net(pc)
    np.random.seed(41)
    got = get_grasp_allobj(pc, score, detect.TEST_PARAMS, [], True)
    np.random.seed(5)
    synthetic.calibrate_region_head(region_net, lambda: _region(region_net, got, pc, feat, detect.GRIPPER_PARAMS))
    return score_net, region_net, (xyz, rgb), kw


def _frozen_class(cache={}):
    """A detector whose networks' proposals are held fixed at the ones of the plain frame.  The synthetic networks (seeded
    weights, calibrated heads) answer a changed cloud with other grasps altogether, so a wall planted behind the grasps of one
    run would stand behind none of the next; everything behind the networks -- ingest, collision filter, approach analysis,
    selection, record -- runs on the frame it is given."""
    from regnet_for_3d_grasping_amd import detect

    class Frozen(detect.GraspDetector):
        def _networks(self, fr):
            if not cache:
                score, sets = super()._networks(fr)
                cache["score"], cache["sets"] = score.clone(), {k: None if v is None else v.clone() for k, v in sets.items()}
            return cache["score"].clone(), {k: None if v is None else v.clone() for k, v in cache["sets"].items()}
    return Frozen


def _run(parts, frame=None, frozen=False, **kw):
    from regnet_for_3d_grasping_amd import detect
    score_net, region_net, own, base = parts
    detector = (_frozen_class() if frozen else detect.GraspDetector)(score_net, region_net, **dict(base, **kw))
    np.random.seed(SEED)
    out = detector.detect(own if frame is None else frame)
    return detector, out, np.random.get_state()


def _same_state(a, b):
    return a[0] == b[0] and np.array_equal(a[1], b[1]) and a[2:] == b[2:]


@pytest.fixture(scope="module")
def plain(parts):
    return _run(parts)


def _restatement(out, source, params, points=None):
    """The restatement on the record's own points and source set (the frames and, with a friction angle, the normals computed by
    the device functions their own tests pin) -> (counts, values, the six derived arrays)."""
    from regnet_for_3d_grasping_amd import detect, eval_collision
    points32 = out["points"].astype(np.float32) if points is None else points
    grasp = torch.from_numpy(out[source]).to(DEV)
    frame, center = eval_collision.grasp_frames(grasp[:, :8].contiguous())
    T = eval_collision.global_to_local(frame, center).cpu().numpy()
    normals, cf = None, 0.0
    if params.friction_deg is not None:
        normals = eval_collision.estimate_normals(torch.from_numpy(points32).to(DEV), radius=params.normal_radius,
                                                  max_nn=params.normal_max_nn).cpu().numpy()
        cf = ref.cos_friction(params.friction_deg)
    box = ref.gripper_box(detect.DEPTH, detect.WIDTH)
    counts, values = ref.approach_ref(points32, normals, T, box, params.standoff, params.contact_depth, cf)
    return counts, values, ref.derived_ref(counts, values, frame.cpu().numpy(), center.cpu().numpy(), params.pad, box[4])


def _keys_equal(out, derived):
    for key, want in derived.items():
        assert out[key].dtype == np.float32 and out[key].shape == want.shape, key
        assert out[key].tobytes() == want.tobytes(), key


def test_without_approach_the_record_is_unchanged(parts, plain):
    from regnet_for_3d_grasping_amd import detect
    _, want, want_state = plain
    _, out, state = _run(parts, approach=None)
    assert tuple(out) == tuple(want) == detect.RESULT_KEYS
    for key in detect.RESULT_KEYS:
        assert out[key].dtype == want[key].dtype and out[key].tobytes() == want[key].tobytes(), key
    assert _same_state(state, want_state)
    assert len(want["grasp_stage3"]) > 1 and len(want["grasp_stage2"]) > 1


@pytest.mark.parametrize("approach", [{}, {"source": "grasp_stage2", "friction_deg": 30.0, "standoff": 0.05, "pad": 0.002}])
def test_the_new_keys_equal_the_restatement(parts, plain, approach):
    from regnet_for_3d_grasping_amd import detect
    detector, out, state = _run(parts, approach=approach)
    assert tuple(out) == detect.RESULT_KEYS + detect.APPROACH_KEYS
    _, want, want_state = plain
    for key in detect.RESULT_KEYS:                              # the rest of the record and numpy's generator: untouched
        assert out[key].dtype == want[key].dtype and out[key].tobytes() == want[key].tobytes(), key
    assert _same_state(state, want_state)
    source = approach.get("source", "grasp_stage3")
    assert detector.approach_source == source and len(out["grasp_clearance"]) == len(out[source]) > 1
    assert out["grasp_pregrasp"].shape == (len(out[source]), 3)
    counts, values, derived = _restatement(out, source, detector.approach)
    _keys_equal(out, derived)
    S = f32(detector.approach.standoff)
    print("%s: %d grasps, free %d, blocked %d, region empty %d, contact > 0: %d" % (
        source, len(counts), (values[:, 2] >= S).sum(), (values[:, 2] < S).sum(), (counts[:, 0] == 0).sum(),
        (derived["grasp_contact"] > 0).sum()))
    assert (out["grasp_width"] > 0).any() and (out["grasp_opening"] <= f32(detect.WIDTH)).all()
    if detector.approach.friction_deg is not None:
        assert (counts[:, 3] > 0).any() and (counts[:, 5] > 0).any()


@pytest.fixture(scope="module")
def walled(parts):
    """The scene leaves every grasp a free approach, so a wall is planted: a disc of points 3 cm behind the palm of some of the
    grasps the detector finds, in the slab their hands sweep.  The wall's points REPLACE the rows of the frame that lie farthest
    from every grasp, so that the frame keeps its size and the resampling draws the same rows.  -> (first record, chosen rows,
    wall points, the frame with the wall)."""
    from regnet_for_3d_grasping_amd import eval_collision, ingest
    _, first, _ = _run(parts, frozen=True, approach={})         # (the first frozen run is the plain frame's: it fills the cache)
    free = np.nonzero(first["grasp_clearance"] >= f32(0.1))[0]
    assert len(free) >= 2
    chosen = free[::3]
    frame, center = eval_collision.grasp_frames(torch.from_numpy(first["grasp_stage3"][chosen]).to(DEV))
    frame, center = frame.cpu().numpy().astype(np.float64), center.cpu().numpy().astype(np.float64)
    grid = np.arange(-3, 4) * 0.004
    offsets = np.array([(-0.09, dy, dz) for dy in grid for dz in grid if dy * dy + dz * dz <= 0.008 ** 2 + 1e-12])
    wall = (center[:, None, :] + np.einsum("bij,kj->bki", frame, offsets)).reshape(-1, 3)
    xyz, rgb = parts[2]
    Tinv = np.linalg.inv(ingest.table_frame_transform())
    T = ingest.table_frame_transform()
    table_xyz = xyz @ T[:3, :3].T + T[:3, 3]
    nearest = np.linalg.norm(table_xyz[:, None, :] - first["grasp_stage3"][None, :, :3].astype(np.float64), axis=2).min(1)
    rows = np.argsort(nearest)[-len(wall):]
    xyz, rgb = xyz.copy(), rgb.copy()
    xyz[rows], rgb[rows] = wall @ Tinv[:3, :3].T + Tinv[:3, 3], 0.5
    with_wall = (xyz, rgb)
    return first, chosen, wall, with_wall


def test_the_frozen_detector_is_the_detector_on_the_plain_frame(parts, plain, walled):
    first = walled[0]
    for key, value in plain[1].items():
        assert first[key].tobytes() == value.tobytes(), key


def test_a_planted_wall_blocks_exactly_the_grasps_the_restatement_names(parts, walled):
    from regnet_for_3d_grasping_amd import approach as approach_mod
    from regnet_for_3d_grasping_amd import detect
    first, chosen, wall, with_wall = walled
    params = approach_mod.ApproachParams()
    S = f32(params.standoff)
    # (1) the same grasps against the same cloud plus the wall: blocked are exactly the ones the restatement names, the chosen
    # ones among them at a retreat of at most 3 cm (a neighbour's wall may stand nearer)
    points32 = np.concatenate([first["points"].astype(np.float32), wall.astype(np.float32)])
    res = approach_mod.analyse(torch.from_numpy(points32).to(DEV), torch.from_numpy(first["grasp_stage3"]).to(DEV), detect.DEPTH,
                               detect.WIDTH, params)
    _, values, derived = _restatement(first, "grasp_stage3", params, points=points32)
    clearance = res.clearance.cpu().numpy()
    assert clearance.tobytes() == derived["grasp_clearance"].tobytes()
    assert np.array_equal(clearance < S, values[:, 2] < S)
    assert (clearance[chosen] < 0.03 + 1e-4).all() and (clearance[chosen] > 0.029).any()      # (a neighbour's wall may stand nearer)
    assert not (first["grasp_clearance"] < S).any()                 # without the wall nothing was blocked
    # (2) the wall in the camera frame, through the detector with the proposals held fixed: the record says what the restatement
    # says on the record's own points, and the grasps with a wall behind them are blocked
    detector, out, _ = _run(parts, frame=with_wall, frozen=True, approach={})
    _, values, derived = _restatement(out, "grasp_stage3", detector.approach)
    _keys_equal(out, derived)
    blocked = out["grasp_clearance"] < S
    assert np.array_equal(blocked, values[:, 2] < S)
    print("wall behind %d of %d grasps: with the wall the detector finds %d grasps, %d of them blocked" % (
        len(chosen), len(first["grasp_clearance"]), len(blocked), blocked.sum()))
    assert blocked.any() and not blocked.all()
    if out["grasp_stage3"].tobytes() == first["grasp_stage3"].tobytes():     # (no wall stands inside a neighbour's closing slab)
        assert blocked[chosen].all()


DISTINCT = {"top_k": 50, "translation_thresh": 1e-4, "rotation_thresh_deg": 0.1}      # every grasp is a distinct one


def test_min_clearance_filters_the_selection(parts, walled):
    from regnet_for_3d_grasping_amd import detect, grasp_select
    with_wall = walled[3]
    bound = 0.05
    _, unfiltered, _ = _run(parts, frame=with_wall, frozen=True, select=DISTINCT, approach={})
    failing = unfiltered["grasp_clearance"] < f32(bound)
    assert failing.any() and not failing.all()
    assert failing[unfiltered["grasp_selected_index"]].any()      # the unfiltered selection holds rows the bound removes
    detector, out, _ = _run(parts, frame=with_wall, frozen=True, select=DISTINCT, approach={"min_clearance": bound})
    assert tuple(out) == detect.RESULT_KEYS + detect.SELECT_KEYS + detect.APPROACH_KEYS
    for key in detect.RESULT_KEYS + detect.APPROACH_KEYS:         # the sets and the analysis are never shortened
        assert out[key].tobytes() == unfiltered[key].tobytes(), key
    index = out["grasp_selected_index"]
    assert index.dtype == np.int64 and len(set(index.tolist())) == len(index) == (~failing).sum()
    assert not failing[index].any()
    assert out["grasp_selected"].tobytes() == out["grasp_stage3"][index].tobytes()        # rows of the FULL source set
    # the selection is pose NMS over the passing rows alone
    passing = np.nonzero(~failing)[0]
    rows, sub = grasp_select.pose_nms(torch.from_numpy(out["grasp_stage3"][passing]).to(DEV), return_index=True, **DISTINCT)
    assert np.array_equal(index, passing[sub.cpu().numpy()]) and rows.cpu().numpy().tobytes() == out["grasp_selected"].tobytes()
    # per object
    _, per, _ = _run(parts, frame=with_wall, frozen=True, select=DISTINCT, segment={"top_k_per_object": 2}, approach={"min_clearance": bound})
    assert tuple(per) == detect.RESULT_KEYS + detect.SEGMENT_SELECT_KEYS + detect.SEGMENT_KEYS + detect.APPROACH_KEYS
    index, objects = per["grasp_selected_index"], per["grasp_selected_object"]
    assert len(index) > 0 and not failing[index].any() and len(per["grasp_object"]) == len(per["grasp_stage3"])
    assert per["grasp_selected"].tobytes() == per["grasp_stage3"][index].tobytes()
    assert np.array_equal(objects, per["grasp_object"][index]) and np.bincount(objects).max() <= 2
    _, per_all, _ = _run(parts, frame=with_wall, frozen=True, select=DISTINCT, segment={"top_k_per_object": 2}, approach={})
    assert per_all["grasp_object"].tobytes() == per["grasp_object"].tobytes()             # grasp_object covers every row
    # min_contact without a friction angle: the contact is 0 everywhere and nothing passes
    _, none, _ = _run(parts, select={"top_k": 5}, approach={"min_contact": 0.5})
    assert none["grasp_selected"].shape == (0, 8) and none["grasp_selected_index"].shape == (0,)


def test_an_empty_source_set(parts):
    from regnet_for_3d_grasping_amd import detect
    # a table far above the scene: the collision filter keeps no grasp of any set
    eval_params = [detect.DEPTH, detect.WIDTH, 10.0, 0, detect.CENTER_NUM]
    for approach in ({"friction_deg": 30.0}, {"min_clearance": 0.05}):
        _, out, _ = _run(parts, eval_params=eval_params, select={"top_k": 5}, approach=approach)
        assert out["grasp_stage3"].shape == (0, 8)
        for key in detect.APPROACH_KEYS[:5]:
            assert out[key].shape == (0,) and out[key].dtype == np.float32, key
        assert out["grasp_pregrasp"].shape == (0, 3) and out["grasp_pregrasp"].dtype == np.float32
        assert out["grasp_selected"].shape == (0, 8) and out["grasp_selected_index"].shape == (0,)
        assert out["grasp_selected_index"].dtype == np.int64


def test_cli_flags_reach_the_params_and_the_file(parts, plain, tmp_path):
    from regnet_for_3d_grasping_amd import approach as approach_mod
    from regnet_for_3d_grasping_amd import detect
    score_net, region_net = parts[:2]
    args = detect.build_parser().parse_args(["--folder", "f", "--load-score-path", "s", "--load-region-path", "r",
                                             "--approach-standoff", "0.08", "--friction-angle", "35", "--min-clearance", "0.02",
                                             "--approach-from", "grasp_stage3"])
    given = detect.approach_from_args(args)
    assert given == {"standoff": 0.08, "friction_deg": 35.0, "min_clearance": 0.02, "source": "grasp_stage3"}
    folder = tmp_path / "scene_data"
    folder.mkdir()
    path = str(folder / "frame.p")
    with open(path, "wb") as f:                                   # a dataset record is analysed too: its cloud is in the table frame
        pickle.dump({"view_cloud": plain[1]["points"].astype(np.float32),
                     "view_cloud_color": plain[1]["colors"].astype(np.float32)}, f)
    detector = detect.GraspDetector(score_net, region_net, approach=given)
    assert detector.approach == approach_mod.ApproachParams(standoff=0.08, friction_deg=35.0, min_clearance=0.02, source="grasp_stage3")
    np.random.seed(SEED)
    printed = io.StringIO()
    with contextlib.redirect_stdout(printed):
        out, saved = detector.detect_file(path)
    lines = printed.getvalue().strip().splitlines()
    free = int((out["grasp_clearance"] >= f32(0.08)).sum())
    assert len(lines) == 4 and lines[3] == "free approach grasp num (grasp_stage3): %d" % free
    with open(saved, "rb") as f:
        record = pickle.load(f)
    assert tuple(record) == detect.RESULT_KEYS + detect.APPROACH_KEYS
    _, _, derived = _restatement(record, "grasp_stage3", detector.approach)
    _keys_equal(record, derived)
