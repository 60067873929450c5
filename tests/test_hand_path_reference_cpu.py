"""The numpy restatement of the hand paths (tests/hand_path_reference.py) held against things it shares no code with, and the host
side of ``regnet_for_3d_grasping_amd.hand_path`` -- no GPU."""
import ctypes
import math

import numpy as np
import pytest

from . import approach_volume_reference as av_ref
from . import hand_path_reference as ref
from . import retreat_reference as fan_ref

f32 = np.float32
NONE = ref.NONE
IDENTITY_L = np.eye(4, dtype=np.float32)[:3].reshape(1, 12)
IDENTITY12 = np.eye(4, dtype=np.float32)[:3].reshape(12)
DYADIC_BOX = (-0.5, 0.5, 0.125, 1.0, 0.75, 0.0)      # x_lo, x_hi, ht, hw, hs, back_x: every constant a dyadic rational
# the corner scene: 48 x 40 x 4 voxels of 0.125 over x in [-4.5, 1.5], y in [-2.5, 2.5]; the obstacle fills x < -2, y > 0.875, a
# wall beside the +y finger (which spans y in (0.75, 1)) whose end face stands 1.5 behind the hand's back face x_lo = -0.5
CDIMS, CORIGIN, CVOXEL = (48, 40, 4), (-4.5, -2.5, -0.25), 0.125
WALL_X, WALL_Y = -2.0, 0.875
H, K, DS, TURN = 0.125, 14, 0.125, 30.0
PIVOT = (-0.5, -1.0, 0.0)                            # the turns are about the hand's rear -y corner, the one far from the wall


def _corner_field(signed):
    """The field of the corner obstacle set by hand: solid where ix < 20 and iy >= 27; outside it the squared distance in voxels
    to the nearest solid voxel, inside it (signed) minus the squared distance to the nearest free one."""
    ix, iy = np.meshgrid(np.arange(CDIMS[0]), np.arange(CDIMS[1]), indexing="xy")       # (ny, nx)
    solid = (ix < 20) & (iy >= 27)
    free2 = np.maximum(ix - 19, 0) ** 2 + np.maximum(27 - iy, 0) ** 2
    depth2 = np.minimum(20 - ix, iy - 26) ** 2
    plane = np.where(solid, -depth2 if signed else 0, free2)
    return np.broadcast_to(plane[None], (CDIMS[2],) + plane.shape).reshape(-1).astype(np.int32)


def _corner_paths():
    from regnet_for_3d_grasping_amd import hand_path
    back = [[-1.0, 0.0, 0.0]]
    # the rear +y corner swings FORWARD and the hand leaves beside the wall / swings BACK into its end face
    away = hand_path.turn_paths(back, (0, 0, 1), PIVOT, -TURN, K * DS, K)
    towards = hand_path.turn_paths(back, (0, 0, 1), PIVOT, TURN, K * DS, K)
    return np.concatenate([hand_path.straight_paths(back, K * DS, K), away, towards])[None]      # (1, 3, K+1, 12)


def _hand_points(spacing):
    """Points of the hand (back || finger of the dyadic box) on a float64 lattice of ``spacing``, faces included."""
    x_lo, x_hi, ht, hw, hs, back_x = DYADIC_BOX
    x, y, z = np.meshgrid(np.arange(x_lo, x_hi + 1e-9, spacing), np.arange(-hw, hw + 1e-9, spacing),
                          np.arange(-ht, ht + 1e-9, spacing), indexing="ij")
    x, y, z = x.reshape(-1), y.reshape(-1), z.reshape(-1)
    hand = (x <= back_x) | (np.abs(y) >= hs)
    return np.stack([x[hand], y[hand], z[hand], np.ones(int(hand.sum()))], axis=0)


def _clearance(rows, points):
    """The smallest true distance from the posed hand points to the obstacle {x <= WALL_X, y >= WALL_Y}, in float64."""
    w = np.asarray(rows, dtype=np.float64).reshape(3, 4) @ points
    return float(np.sqrt(np.maximum(w[0] - WALL_X, 0.0) ** 2 + np.maximum(WALL_Y - w[1], 0.0) ** 2).min())


def _continuous_pose(angle_deg, t):
    """The pose at path parameter t (metres of translation) of the path turning by ``angle_deg`` over K * DS, in float64."""
    a = math.radians(angle_deg) * t / (K * DS)
    c, s, (px, py, _) = math.cos(a), math.sin(a), PIVOT
    return np.array([[c, -s, 0, px - (c * px - s * py) - t], [s, c, 0, py - (s * px + c * py)], [0, 0, 1, 0]])


def test_translation_only_paths_are_the_retreat_fan_where_every_sum_is_exact():
    """Identity rotation; every coordinate, box constant, h and ds a multiple of 2^-10 below 8: the fan's ``x + (k ds) d`` then
    ``L`` and the path's one affine map per waypoint round nowhere, so the two restatements read the same voxels."""
    from regnet_for_3d_grasping_amd import hand_path
    dims, origin, voxel = (40, 48, 4), (-4.0, -1.5, -0.25), 0.125
    field = np.random.default_rng(11).integers(0, 500, size=dims[0] * dims[1] * dims[2]).astype(np.int32)
    dirs = np.array([[-1, 0, 0], [-0.5, 0.75, 0], [0.25, -1, 0.5], [0, 0, 0]], dtype=np.float32)
    steps, ds = 24, 0.125
    local = hand_path.straight_paths(dirs, steps * ds, steps)
    assert local.shape == (4, 25, 12) and local.dtype == np.float32
    P = ref.compose_ref(IDENTITY_L, local)
    assert np.array_equal(P[0], local)
    # exactness: the float32 positions equal a float64 evaluation, for the path's map and for the fan's formula
    xv, yv, zv = av_ref.lattice_samples(DYADIC_BOX, 0.0, H, 0.5)
    x, y, z = (a.reshape(-1) for a in np.meshgrid(xv, yv, zv, indexing="ij"))
    for r in range(4):
        for k in (0, 1, 7, 24):
            exact = np.stack([x, y, z]).astype(np.float64) + (k * ds) * dirs[r].astype(np.float64)[:, None]
            got = ref._apply(P[0, r, k], (x, y, z))
            t = f32(k) * f32(ds)
            fan = [x + t * dirs[r, 0], y + t * dirs[r, 1], z + t * dirs[r, 2]]
            for i in range(3):
                assert got[i].dtype == np.float32 and np.array_equal(got[i].astype(np.float64), exact[i])
                assert np.array_equal(fan[i].astype(np.float64), exact[i])
    for outside in (0, 1):
        want_p, want_r = fan_ref.fan_ref(field, dims, origin, voxel, outside, IDENTITY_L, DYADIC_BOX, H, 0.5, dirs, steps, ds, 3, False)
        profile, result = ref.path_ref(field, dims, origin, voxel, outside, P, DYADIC_BOX, H, 0.5, 3, False)
        assert np.array_equal(profile, want_p) and np.array_equal(result, want_r)
        assert result[0, 2, 3] > 0 and result[0, 3, 3] == 0                      # the third hand leaves the volume on its way
    assert len(set(profile[0, 3].tolist())) == 1 and len(set(profile[0, 0].tolist())) > 1      # the zero direction stands still


def test_a_wall_beside_one_finger_turning_away_is_free_and_turning_towards_is_shorter():
    """The corner scene.  Straight back, the +y finger meets the wall's end face after 1.5; turning away (the rear +y corner
    swings forward, the fingers slide past the face) the whole path is free; turning towards, the rear corner reaches the face
    sooner.  The geometric free lengths come from a float64 evaluation of the continuous motion over a fine point set of the
    hand.  The restatement's are quantised as the fan's: the hand's outermost samples sit up to a lattice step h inside its
    faces, the length counts whole steps -- here ``ds_equiv``, the farthest the hand moves in one step, ``disp`` -- and a
    nearest-voxel lookup of a cell-centred sample places a face within 1.5 voxels: |free - truth| <= h + ds_equiv + 1.5 voxels.
    The motion meets the face head-on (the rear corner's speed towards it is at least the translation's), so the bound holds in
    the path's own parameter."""
    field = _corner_field(False)
    P = _corner_paths()
    profile, result = ref.path_ref(field, CDIMS, CORIGIN, CVOXEL, 0, P, DYADIC_BOX, H, 0.5, 1, False)
    disp = ref.disp_ref(P, DYADIC_BOX)
    assert result[0, :, 3].tolist() == [0, 0, 0]                                 # the paths stay inside the volume
    points = _hand_points(1.0 / 32)
    truth = []
    for angle in (0.0, -TURN, TURN):
        ts = np.arange(0.0, K * DS + 1e-9, DS / 32)
        hit = [t for t in ts if _clearance(_continuous_pose(angle, t), points) <= 0.0]
        truth.append(hit[0] if hit else K * DS)
    assert truth[0] == 1.5 and truth[1] == K * DS and truth[2] < 1.3             # the scene itself, without the restatement
    free = result[0, :, 0] * DS
    for r in range(3):
        bound = H + float(disp[0, r].max()) + 1.5 * CVOXEL
        assert abs(free[r] - truth[r]) <= bound, (r, free[r], truth[r], bound)
    assert result[0, 0, 0] < K and result[0, 1, 0] == K and result[0, 2, 0] < result[0, 0, 0]
    assert fan_ref.pick_ref(result)[0].tolist() == [1, K, result[0, 1, 1], 0]
    assert profile[0, 0, 0] == profile[0, 1, 0] == profile[0, 2, 0]              # waypoint 0 is the final pose for every path


def test_disp_of_a_translation_is_the_step_and_of_a_rotation_the_farthest_corners_chord():
    from regnet_for_3d_grasping_amd import hand_path
    d = np.array([[-0.6, 0.0, 0.8], [1.0, 2.0, -2.0]])
    local = hand_path.straight_paths(d, 0.7, 7)
    disp = ref.disp_ref(ref.compose_ref(np.array([[0.36, 0.48, -0.8, 0.01, -0.8, 0.6, 0.0, -0.02, 0.48, 0.64, 0.6, 0.015]]), local),
                        DYADIC_BOX)
    # a pure translation by 0.1 |d|: a few roundings of coordinates of size 1 -- an ulp of 1 is 1.2e-7
    assert np.abs(disp[0, 0] - 0.1).max() < 1e-6 and np.abs(disp[0, 1] - 0.3).max() < 1e-6
    pivot = (-0.25, -0.5, 0.0625)
    turn = hand_path.turn_paths([[0.0, 0.0, 0.0]], (0, 0, 1), pivot, 40.0, 0.0, 8)
    disp = ref.disp_ref(turn[None], DYADIC_BOX)
    corners = [(x, y) for x in DYADIC_BOX[:2] for y in (-1.0, 1.0)]
    radius = max(math.hypot(x - pivot[0], y - pivot[1]) for x, y in corners)
    chord = 2.0 * radius * math.sin(math.radians(5.0) / 2.0)
    assert np.abs(disp[0, 0] - chord).max() < 1e-6, (disp, chord)
    per_grasp = (DYADIC_BOX[0], np.array([0.5, 0.0], dtype=np.float32)) + DYADIC_BOX[2:]      # a shorter hand turns less far
    both = ref.disp_ref(np.repeat(turn[None], 2, axis=0), per_grasp)
    assert np.array_equal(both[0], disp[0]) and (both[1] < both[0]).all()
    bad = turn[None].copy()
    bad[0, 0, 3, 5] = np.nan                                                                  # a NaN row at waypoint 3
    got = ref.disp_ref(bad, DYADIC_BOX)
    assert np.isnan(got[0, 0, 2:4]).all() and np.isfinite(np.delete(got[0, 0], [2, 3])).all()


def test_the_certificate_is_conservative_on_the_corner_scene():
    """Signed field, ``min_margin`` one voxel.  Every certified segment is resampled densely: 32 linear blends of the two poses'
    rows (the chord the certificate assumes), hand points on a lattice of h / 4, and the TRUE distance to the obstacle is at
    least ``min_margin`` everywhere.  The scene certifies at least half of the steps the profile calls free -- otherwise this
    would show nothing; that is a condition on the scene, checked on the restatement alone."""
    from regnet_for_3d_grasping_amd import hand_path
    min_margin = 0.125
    field = _corner_field(True)
    thresh = hand_path.threshold_word(min_margin, CVOXEL, True)
    assert thresh == 3                                                           # (sqrt(3) - 0.5) voxels is the first >= one voxel
    P = _corner_paths()
    profile, result = ref.path_ref(field, CDIMS, CORIGIN, CVOXEL, 0, P, DYADIC_BOX, H, 0.5, thresh, True)
    disp = ref.disp_ref(P, DYADIC_BOX)
    slack = ref.default_slack(H, CVOXEL)
    assert slack == (H + CVOXEL) * math.sqrt(3.0) / 2.0
    certified = ref.certified_ref(profile, disp, CVOXEL, True, slack, min_margin)
    free = result[0, :, 0]
    assert (certified[0] <= free).all() and (2 * certified[0] >= free).all() and (free > 0).all(), (certified, free)
    points = _hand_points(H / 4)
    for r in range(3):
        for k in range(1, int(certified[0, r]) + 1):
            a, b = P[0, r, k - 1].astype(np.float64), P[0, r, k].astype(np.float64)
            for i in range(33):
                s = i / 32.0
                assert _clearance((1.0 - s) * a + s * b, points) >= min_margin, (r, k, i)
    # more slack certifies less, none at all with a slack beyond every margin; a NaN displacement ends the prefix
    assert (ref.certified_ref(profile, disp, CVOXEL, True, 2 * slack, min_margin) <= certified).all()
    assert (ref.certified_ref(profile, disp, CVOXEL, True, 100.0, min_margin) == 0).all()
    broken = disp.copy()
    broken[0, 1, 2] = np.nan
    assert ref.certified_ref(profile, broken, CVOXEL, True, slack, min_margin)[0].tolist() == [certified[0, 0], 2, certified[0, 2]]


def test_generators_params_and_the_threshold_word():
    from regnet_for_3d_grasping_amd import approach, hand_path, retreat
    assert hand_path.threshold_word is retreat.threshold_word
    assert approach.PathParams is hand_path.PathParams and approach.PathCheck is hand_path.PathCheck
    p = hand_path.PathParams()
    assert (p.length, p.steps, p.tilt_deg, p.turn_deg, tuple(p.pivot), p.paths, p.min_margin, p.step) == \
        (0.10, 20, 25.0, 20.0, (0, 0, 0), None, 0.0, None)
    assert hand_path.PathParams.WORD == "paths" and hand_path.PathParams.coerce({"steps": 7}).steps == 7
    with pytest.raises(TypeError, match="^paths must be None, a dict or a PathParams$"):
        hand_path.PathParams.coerce(3)
    for bad in ({"length": -0.1}, {"length": float("nan")}, {"steps": 0}, {"steps": 65}, {"steps": 2.5}, {"tilt_deg": 91.0},
                {"turn_deg": 181.0}, {"turn_deg": float("nan")}, {"pivot": (0, 0)}, {"pivot": (0, 0, float("inf"))},
                {"paths": np.zeros((17, 3, 12))}, {"paths": np.zeros((2, 1, 12))}, {"paths": np.zeros((2, 66, 12))},
                {"paths": np.zeros((3, 12))}, {"paths": np.zeros((2, 3, 16))}, {"min_margin": float("nan")}, {"step": 0.0},
                {"step": 1e-60}):
        with pytest.raises(ValueError, match="paths: %s" % next(iter(bad))):
            hand_path.PathParams(**bad)
    assert hand_path.PathParams(paths=np.zeros((2, 5, 3, 12))).paths.shape == (2, 5, 3, 12)
    # the default set: 9 paths, the fan's five directions straight and in its order, then +-turn about z, then +-turn about y
    paths = hand_path.default_paths({"steps": 10, "length": 0.2, "turn_deg": 30.0, "pivot": (0.05, 0.0, 0.0)})
    assert paths.shape == (9, 11, 12) and paths.dtype == np.float32
    assert np.array_equal(paths[:, 0].view(np.uint32), np.broadcast_to(IDENTITY12, (9, 12)).copy().view(np.uint32))   # bit for bit
    rows = paths.reshape(9, 11, 3, 4)
    c, s = math.cos(math.radians(25.0)), math.sin(math.radians(25.0))
    fan = np.array([[-1, 0, 0], [-c, 0, s], [-c, 0, -s], [-c, s, 0], [-c, -s, 0]])
    assert np.array_equal(rows[:5, :, :, :3], np.broadcast_to(np.eye(3, dtype=np.float32), (5, 11, 3, 3)))
    assert np.allclose(rows[:5, 10, :, 3], 0.2 * fan, atol=1e-7) and np.allclose(rows[:5, 5, :, 3], 0.1 * fan, atol=1e-7)
    half = math.radians(30.0)
    for r, (axis, sign) in zip(range(5, 9), (("z", 1), ("z", -1), ("y", 1), ("y", -1))):
        rot = rows[r, 10, :, :3].astype(np.float64)
        a = sign * half
        want = np.array([[math.cos(a), -math.sin(a), 0], [math.sin(a), math.cos(a), 0], [0, 0, 1]]) if axis == "z" else \
            np.array([[math.cos(a), 0, math.sin(a)], [0, 1, 0], [-math.sin(a), 0, math.cos(a)]])
        assert np.allclose(rot, want, atol=1e-7), r
        # the pivot, moved by the translation alone: it is the fixed point of the turn
        pivot = np.array([0.05, 0.0, 0.0])
        assert np.allclose(rot @ pivot + rows[r, 10, :, 3], pivot + 0.2 * fan[0], atol=1e-7)
        assert np.allclose(rows[r, 5, :, :3].astype(np.float64) @ rows[r, 5, :, :3].astype(np.float64), rot, atol=1e-6)   # half the angle half way
    assert np.array_equal(hand_path.default_paths()[:, 0].view(np.uint32), np.broadcast_to(IDENTITY12, (9, 12)).copy().view(np.uint32))
    assert hand_path.default_paths().shape == (9, 21, 12)
    with pytest.raises(ValueError, match="paths: the turn's axis"):
        hand_path.turn_paths([[1, 0, 0]], (0, 0, 0), (0, 0, 0), 10.0, 0.1, 4)
    with pytest.raises(ValueError, match="paths: K must be"):
        hand_path.straight_paths([[1, 0, 0]], 0.1, 65)


def test_compose_ref_is_the_matrix_product():
    from regnet_for_3d_grasping_amd import hand_path
    L = np.array([[0.36, 0.48, -0.8, 0.01, -0.8, 0.6, 0.0, -0.02, 0.48, 0.64, 0.6, 0.015]], dtype=np.float32)
    local = hand_path.default_paths({"steps": 4})
    P = ref.compose_ref(L, local)
    full = np.concatenate([L.reshape(3, 4).astype(np.float64), [[0, 0, 0, 1]]])
    for r in range(9):
        for k in range(5):
            m = np.concatenate([local[r, k].reshape(3, 4).astype(np.float64), [[0, 0, 0, 1]]])
            assert np.allclose(P[0, r, k].reshape(3, 4), (full @ m)[:3], atol=1e-6)
    assert np.array_equal(P[0, :, 0], np.broadcast_to(L, (9, 12)))                # waypoint 0 is the final grasp pose itself


def test_the_header_declares_the_entry_points_and_they_refuse_before_any_launch():
    """The argument checks come before any launch, so they run without a GPU; their order is the fan's."""
    from regnet_for_3d_grasping_amd import _lib
    from regnet_for_3d_grasping_amd.csrc import build
    from .test_retreat_reference_cpu import _status_codes
    codes = _status_codes()
    assert dict(build.SOURCES)["hand_path.hip"] == ["-ffp-contract=off"] and build.NO_VGPR_SPILL["hand_path.o"] == ["hand_path_"]
    origin = (ctypes.c_float * 3)(0.0, 0.0, 0.0)
    fake = ctypes.c_void_p(16)                       # never read: every call below returns before a launch
    for name in ("regnet_grasp_path_check_f32", "regnet_grasp_path_check_signed_f32"):
        assert _lib.PARAMS[name] == ["field", "nx", "ny", "nz", "origin3", "voxel", "outside", "P", "B", "R", "K", "x_lo", "x_hi",
                                     "x_hi_per_grasp", "half_thickness", "half_width", "half_space", "back_x", "step", "x_extent",
                                     "thresh", "profile", "result", "disp", "stream"]
        fn = getattr(_lib.lib, name)

        def call(dims=(8, 8, 8), voxel=0.01, outside=0, B=1, step=0.01, R=5, K=20, field=fake, org=origin, P=fake, result=fake):
            return fn(field, *dims, org, voxel, outside, P, B, R, K, -0.05, 0.06, None, 0.01, 0.05, 0.04, -0.01, step, 0.06, 1,
                      None, result, None, None)

        assert call(B=0) == codes["OK"] and call(B=0, field=None, org=None, P=None, result=None) == codes["OK"]
        for bad in (dict(B=-1), dict(outside=2), dict(outside=-1), dict(R=0), dict(K=0), dict(dims=(0, 8, 8))):
            assert call(**bad) == codes["SHAPE"], bad
        for bad in (dict(dims=(1025, 8, 8)), dict(B=1 << 31), dict(voxel=0.0), dict(step=float("nan")), dict(R=17), dict(K=65),
                    dict(B=(1 << 28) // (5 * 21) + 1), dict(step=1e-9)):
            assert call(**bad) == codes["UNSUPPORTED"], bad
        assert call(B=0, R=16, K=64) == codes["OK"]
        assert call(R=0, dims=(1025, 8, 8)) == codes["SHAPE"] and call(B=0, K=65) == codes["UNSUPPORTED"]   # the order of the checks
        assert call(B=1 << 31, voxel=0.0, R=17) == codes["UNSUPPORTED"] and call(field=None, K=65) == codes["UNSUPPORTED"]
        for bad in (dict(field=None), dict(org=None), dict(P=None), dict(result=None)):
            assert call(**bad) == codes["NULL"], bad


def test_the_detectors_path_params_and_cli_flags():
    """``PathApproachParams`` carries ``paths`` / ``min_path``; ``ApproachParams``' own constructor is what it was."""
    import inspect
    from regnet_for_3d_grasping_amd import approach, detect, hand_path
    P, Q = approach.ApproachParams, approach.PathApproachParams
    assert issubclass(Q, P) and P().paths is None and P().min_path is None and not P().filters()
    assert list(inspect.signature(P).parameters)[-2:] == ["retreat", "min_retreat"]
    names = list(inspect.signature(Q).parameters)
    assert names[-4:] == ["retreat", "min_retreat", "paths", "min_path"]
    assert [inspect.signature(Q).parameters[n].kind.name for n in names[-4:]] == ["KEYWORD_ONLY"] * 4
    with pytest.raises(TypeError):
        P(space="volume", field=True, paths=True)
    on = P.coerce({"space": "volume", "field": True, "paths": True})
    assert type(on) is Q and on.paths == hand_path.PathParams() and not on.filters()
    assert P.coerce({"space": "volume", "field": True, "paths": {"steps": 5}, "min_path": 0.05}).filters()
    assert type(P.coerce({"space": "volume", "field": True})) is P and P.coerce(on) is on and Q.coerce(on) is on
    for bad in (dict(paths=True), dict(space="volume", paths=True), dict(field=True, space="volume", min_path=0.05),
                dict(min_path=0.05), dict(space="volume", field=True, paths=True, min_path=-0.01),
                dict(space="volume", field=True, paths={"min_margin": -0.001})):
        with pytest.raises(ValueError, match="approach: "):
            P.coerce(bad)
    assert Q(space="volume", field=True, field_signed=True, paths={"min_margin": -0.001}).paths.min_margin == -0.001
    assert Q(space="volume", field=True, paths=False) == Q(space="volume", field=True)
    assert Q(space="volume", field=True, paths=True, retreat=True).retreat is not None          # beside the fan, independent
    from regnet_for_3d_grasping_amd import approach_volume
    with pytest.raises(ValueError, match="params.paths reads a distance field"):                 # before anything is touched
        approach_volume.analyse_volume(None, None, 0.06, 0.08, on)
    parser = detect.build_parser()
    required = ["--folder", "f", "--load-score-path", "s", "--load-region-path", "r"]
    assert detect.approach_from_args(parser.parse_args(required)) is None
    given = detect.approach_from_args(parser.parse_args(required + ["--approach-space", "volume", "--approach-paths"]))
    assert given == {"space": "volume", "paths": True, "field": True} and P.coerce(given).paths == hand_path.PathParams()
    args = parser.parse_args(required + ["--approach-space", "volume", "--path-turn", "30", "--path-length", "0.08", "--path-steps",
                                         "16", "--path-pivot", "0.01", "0", "-0.02", "--min-path", "0.05"])
    given = detect.approach_from_args(args)
    assert given == {"space": "volume", "field": True, "min_path": 0.05,
                     "paths": {"turn_deg": 30.0, "length": 0.08, "steps": 16, "pivot": (0.01, 0.0, -0.02)}}
    p = P.coerce(given)
    assert (p.paths.turn_deg, p.paths.length, p.paths.steps, p.paths.pivot, p.min_path) == (30.0, 0.08, 16, (0.01, 0.0, -0.02), 0.05)
    assert detect.APPROACH_PATH_KEYS == ("grasp_path_index", "grasp_path_steps", "grasp_path_certified", "grasp_path_margin",
                                         "grasp_path_pose")
