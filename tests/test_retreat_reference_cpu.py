"""The numpy restatement of the retreat fan (tests/retreat_reference.py) held against things it shares no code with, and the host
side of ``regnet_for_3d_grasping_amd.retreat`` -- no GPU."""
import ctypes
import math

import numpy as np
import pytest

from . import edt_reference as edt_ref
from . import retreat_reference as ref
from . import sdf_reference as sdf_ref

f32 = np.float32
NONE = ref.NONE
IDENTITY_L = np.eye(4, dtype=np.float32)[:3].reshape(1, 12)
TURNED = np.array([[0.36, 0.48, -0.8, 0.01], [-0.8, 0.6, 0.0, -0.02], [0.48, 0.64, 0.6, 0.015]])   # a rotation and a shift
DYADIC_BOX = (-0.5, 0.5, 0.125, 1.0, 0.75, 0.0)      # x_lo, x_hi, ht, hw, hs, back_x: every constant a dyadic rational
FAN = np.array([[-1, 0, 0], [-0.5, 0, 0.75], [-0.5, 0.75, 0], [0.25, -1, 0.5]], dtype=np.float32)


def test_step_0_of_every_direction_is_the_hand_margin_at_standoff_0():
    """``edt_reference.margin_ref`` with standoff 0 shares only the lookup with the restatement: its hand minimum is the
    profile's step 0, whatever the direction, on a random field of ragged dims under an oblique transform."""
    dims, origin, voxel = (37, 29, 23), (-0.30, -0.25, -0.20), 0.02
    rng = np.random.default_rng(5)
    field = rng.integers(0, 500, size=dims[0] * dims[1] * dims[2]).astype(np.int32)
    box = (-0.05, 0.06, 0.01, 0.05, 0.04, -0.01)
    L = np.stack([TURNED.reshape(12), IDENTITY_L[0], TURNED.reshape(12)]).astype(np.float32)
    L[2, 3::4] += f32(0.2)                           # the third hand leaves the volume in part
    for outside in (0, 1):
        margins, counts = edt_ref.margin_ref(field, dims, origin, voxel, outside, L, box, 0.0, 0.01, 0.06)
        assert counts[2, 1] > 0 and counts[0, 1] == 0
        profile, result = ref.fan_ref(field, dims, origin, voxel, outside, L, box, 0.01, 0.06, FAN, 3, 0.013, 1, False)
        for r in range(len(FAN)):
            assert np.array_equal(profile[:, r, 0], margins[:, 0]), (outside, r)
        assert not np.array_equal(profile[:, 0, 1:], profile[:, 1, 1:])       # ... and the later steps do depend on it


def _wall_field(dims, wall):
    """The unsigned field of a wall that fills every voxel with ix < wall, set by hand: (ix - (wall - 1))^2 in front of it."""
    ix = np.arange(dims[0])
    line = np.where(ix < wall, 0, (ix - (wall - 1)) ** 2)
    return np.broadcast_to(line[None, None, :], (dims[2], dims[1], dims[0])).reshape(-1).astype(np.int32)


def test_a_wall_behind_the_hand_gives_the_known_free_length_and_a_longer_one_tilted_away():
    """The hand of the dyadic box at the origin, identity transform; the wall's face is the plane x = -2, D = 1.5 behind the
    hand's back face x_lo = -0.5.  Straight back the hand is free for D; along a direction tilted by 60 degrees it reaches the wall
    after D / cos = 3.0, the whole path.  The restatement's free length is quantised: the rearmost samples sit up to one lattice
    step h in front of the back face, the length counts whole steps ds, and a nearest-voxel lookup of a sample places the wall
    within a voxel, half a voxel more for the cell-centred sample: |free_length - truth| <= h + ds + 1.5 voxels."""
    dims, origin, voxel = (40, 48, 4), (-4.0, -1.5, -0.25), 0.125
    field = _wall_field(dims, 16)                    # the face at -4 + 16 * 0.125 = -2
    h, K, ds = 0.125, 24, 0.125
    cos, sin = 0.5, math.sqrt(0.75)
    dirs = np.array([[-1, 0, 0], [-cos, sin, 0]], dtype=np.float32)
    profile, result = ref.fan_ref(field, dims, origin, voxel, 0, IDENTITY_L, DYADIC_BOX, h, 0.5, dirs, K, ds, 1, False)
    bound = h + ds + 1.5 * voxel
    straight, tilted = result[0, 0, 0] * ds, result[0, 1, 0] * ds
    assert abs(straight - 1.5) <= bound, straight
    assert abs(tilted - min(1.5 / cos, K * ds)) <= bound, tilted
    assert tilted > straight
    assert result[0, :, 3].tolist() == [0, 0]        # the paths stay inside the volume
    assert profile[0, 0, 0] == profile[0, 1, 0] == (28 - 15) ** 2             # the rearmost sample's voxel, ix = 28 at x = -0.4375, from the wall's last, 15
    assert ref.pick_ref(result)[0].tolist() == [1, result[0, 1, 0], result[0, 1, 1], 0]


def test_a_zero_direction_and_a_zero_step_give_a_constant_profile():
    dims, origin, voxel = (37, 29, 23), (-0.30, -0.25, -0.20), 0.02
    field = np.random.default_rng(9).integers(1, 900, size=dims[0] * dims[1] * dims[2]).astype(np.int32)
    box = (-0.05, 0.06, 0.01, 0.05, 0.04, -0.01)
    dirs = np.array([[0, 0, 0], [-1, 0, 0]], dtype=np.float32)
    profile, result = ref.fan_ref(field, dims, origin, voxel, 0, TURNED.reshape(1, 12), box, 0.01, 0.06, dirs, 7, 0.01, 1, False)
    assert (profile[0, 0] == profile[0, 0, 0]).all() and not (profile[0, 1] == profile[0, 1, 0]).all()
    profile, _ = ref.fan_ref(field, dims, origin, voxel, 0, TURNED.reshape(1, 12), box, 0.01, 0.06, dirs, 7, 0.0, 1, False)
    assert (profile[0] == profile[0, 0, 0]).all()


def test_the_prefix_rule_and_the_pick():
    dims, origin, voxel = (40, 48, 4), (-4.0, -1.5, -0.25), 0.125
    field = _wall_field(dims, 16)
    dirs = np.array([[-1, 0, 0]], dtype=np.float32)
    # free space again behind a wall four voxels thick: a later free step after a blocked one does not extend the prefix
    field = field.reshape(dims[2], dims[1], dims[0]).copy()
    field[:, :, 0:12] = 9                            # (at step 24 the hand's eight voxel columns are ix = 4 .. 11)
    profile, result = ref.fan_ref(field.reshape(-1), dims, origin, voxel, 0, IDENTITY_L, DYADIC_BOX, 0.125, 0.5, dirs, 24, 0.125, 1,
                                  False)
    free = int(result[0, 0, 0])
    assert profile[0, 0, free + 1] < 1 and profile[0, 0, 24] >= 1 and free == 12
    assert result[0, 0, 1] == profile[0, 0, 1:free + 1].min() and result[0, 0, 2] == 0
    rows = np.array([[[3, 5, 0, 0], [4, 1, 0, 0], [4, 2, 0, 0], [4, 2, 0, 0], [0, NONE, 0, 0]],     # steps, then margin, then r
                     [[0, NONE, 0, 0], [0, NONE, 0, 0], [0, NONE, 0, 0], [0, NONE, 0, 0], [0, NONE, 0, 0]]], dtype=np.int32)
    assert ref.pick_ref(rows).tolist() == [[2, 4, 2, 0], [0, 0, NONE, 0]]


@pytest.mark.parametrize("signed", [False, True])
def test_the_threshold_word_at_its_boundary(signed):
    from regnet_for_3d_grasping_amd import retreat
    voxel = 0.004
    metres = (lambda w: sdf_ref.metres_signed_ref(np.array([w], dtype=np.int32), voxel)[0]) if signed else \
        (lambda w: edt_ref.metres_ref(np.array([w], dtype=np.int32), voxel)[0])
    words = ([-400, -9, -2, -1, 1, 2, 9, 400] if signed else [1, 2, 9, 400])
    for w in words:
        m = metres(w)
        assert retreat.word_metres(w, voxel, signed) == m
        below = -1 if (signed and w == 1) else w - 1
        above = 1 if (signed and w == -1) else w + 1
        assert metres(below) < m < metres(above)
        # exactly at the word's value the word is free; one float32 above it the next word is the threshold
        assert retreat.threshold_word(float(m), voxel, signed) == w == ref.threshold_ref(float(m), voxel, signed)
        up = float(np.nextafter(m, f32(np.inf)))
        assert retreat.threshold_word(up, voxel, signed) == above == ref.threshold_ref(up, voxel, signed)
    assert retreat.threshold_word(0.0, voxel, signed) == (1 if signed else 0) == ref.threshold_ref(0.0, voxel, signed)
    assert retreat.threshold_word(1e9, voxel, signed) == NONE
    if signed:
        assert retreat.threshold_word(-1e9, voxel, signed) == -3 * 1023 * 1023      # (-NONE converts to -inf, below any finite bound)
        assert retreat.threshold_word(-0.003, voxel, True) == -1 == ref.threshold_ref(-0.003, voxel, True)


def test_params_validation():
    from regnet_for_3d_grasping_amd import approach, retreat
    p = retreat.RetreatParams()
    assert (p.length, p.steps, p.tilt_deg, p.up, p.directions, p.min_margin, p.step) == (0.10, 20, 25.0, None, None, 0.0, None)
    assert approach.RetreatParams is retreat.RetreatParams and approach.RetreatFan is retreat.RetreatFan
    assert retreat.RetreatParams.coerce({"steps": 7}).steps == 7 and retreat.RetreatParams.coerce(None) is None
    with pytest.raises(TypeError, match="^retreat must be None, a dict or a RetreatParams$"):
        retreat.RetreatParams.coerce(3)
    for bad in ({"length": -0.1}, {"length": float("nan")}, {"steps": 0}, {"steps": 65}, {"steps": 2.5}, {"tilt_deg": 91.0},
                {"up": (0, 0, 0)}, {"up": (1, 2)}, {"directions": np.zeros((17, 3))}, {"directions": np.zeros((3,))},
                {"directions": np.zeros((2, 2, 4))}, {"min_margin": float("nan")}, {"step": 0.0}, {"step": 1e-60}):
        with pytest.raises(ValueError, match="retreat: %s" % next(iter(bad))):
            retreat.RetreatParams(**bad)
    P = approach.ApproachParams
    assert P().retreat is None and P().min_retreat is None and not P().filters()
    on = P(space="volume", field=True, retreat=True)
    assert on.retreat == retreat.RetreatParams() and not on.filters()
    assert P(space="volume", field=True, retreat={"steps": 5}, min_retreat=0.05).filters()
    for bad in (dict(retreat=True), dict(space="volume", retreat=True), dict(field=True, space="volume", min_retreat=0.05),
                dict(min_retreat=0.05), dict(space="volume", field=True, retreat=True, min_retreat=-0.01),
                dict(space="volume", field=True, retreat={"min_margin": -0.001})):
        with pytest.raises(ValueError, match="approach: "):
            P(**bad)
    assert P(space="volume", field=True, field_signed=True, retreat={"min_margin": -0.001}).retreat.min_margin == -0.001
    off = P(space="volume", field=True, retreat=False)                        # False is off, as None is
    assert off.retreat is None and off == P(space="volume", field=True)
    # keyword-only: the positional order of the fields that were there is what it was
    import inspect
    names = list(inspect.signature(P).parameters)
    assert names[-4:] == ["field_signed", "field_max_distance", "retreat", "min_retreat"]
    assert [inspect.signature(P).parameters[n].kind.name for n in names[-2:]] == ["KEYWORD_ONLY"] * 2
    assert P(None, 0.1, 0.005, None, 0.01, 30, 0.005, None, None, "volume", "free", None, 0.0, True, None, True, 0.1).field_max_distance == 0.1
    from regnet_for_3d_grasping_amd import approach_volume
    with pytest.raises(ValueError, match="params.retreat reads a distance field"):          # before anything is touched
        approach_volume.analyse_volume(None, None, 0.06, 0.08, on)


def test_cli_flags_reach_the_params():
    from regnet_for_3d_grasping_amd import approach, detect
    parser = detect.build_parser()
    required = ["--folder", "f", "--load-score-path", "s", "--load-region-path", "r"]
    assert detect.approach_from_args(parser.parse_args(required)) is None
    given = detect.approach_from_args(parser.parse_args(required + ["--approach-space", "volume", "--approach-retreat"]))
    assert given == {"space": "volume", "retreat": True, "field": True}
    assert approach.ApproachParams.coerce(given).retreat == approach.RetreatParams()
    args = parser.parse_args(required + ["--approach-space", "volume", "--retreat-length", "0.08", "--retreat-steps", "16",
                                         "--retreat-tilt", "30", "--retreat-up", "0", "0", "1", "--min-retreat", "0.05"])
    given = detect.approach_from_args(args)
    assert given == {"space": "volume", "field": True, "min_retreat": 0.05,
                     "retreat": {"length": 0.08, "steps": 16, "tilt_deg": 30.0, "up": (0.0, 0.0, 1.0)}}
    p = approach.ApproachParams.coerce(given)
    assert (p.retreat.length, p.retreat.steps, p.retreat.tilt_deg, p.retreat.up, p.min_retreat) == (0.08, 16, 30.0, (0.0, 0.0, 1.0), 0.05)
    assert detect.APPROACH_RETREAT_KEYS == ("grasp_retreat_index", "grasp_retreat_length", "grasp_retreat_margin",
                                            "grasp_retreat_direction", "grasp_retreat_pregrasp", "grasp_retreat_steps")


def test_the_header_declares_the_entry_points_and_they_refuse_before_any_launch():
    """The argument checks come before any launch, so they run without a GPU."""
    from regnet_for_3d_grasping_amd import _lib
    codes = _status_codes()
    origin = (ctypes.c_float * 3)(0.0, 0.0, 0.0)
    fake = ctypes.c_void_p(16)                       # never read: every call below returns before a launch
    for name in ("regnet_grasp_retreat_fan_f32", "regnet_grasp_retreat_fan_signed_f32"):
        assert _lib.PARAMS[name][-1] == "stream" and len(_lib.PARAMS[name]) == 27
        fn = getattr(_lib.lib, name)

        def call(dims=(8, 8, 8), voxel=0.01, outside=0, B=1, step=0.01, stride=0, R=5, K=20, ds=0.005, field=fake, org=origin,
                 L=fake, dirs=fake, result=fake):
            return fn(field, *dims, org, voxel, outside, L, B, -0.05, 0.06, None, 0.01, 0.05, 0.04, -0.01, step, 0.06, dirs, stride,
                      R, K, ds, 1, None, result, None)

        assert call(B=0) == codes["OK"]
        for bad in (dict(B=-1), dict(outside=2), dict(R=0), dict(K=0), dict(stride=-3), dict(dims=(0, 8, 8))):
            assert call(**bad) == codes["SHAPE"], bad
        for bad in (dict(dims=(1025, 8, 8)), dict(B=1 << 31), dict(voxel=0.0), dict(step=float("nan")), dict(R=17), dict(K=65),
                    dict(B=(1 << 28) // (5 * 21) + 1), dict(ds=-0.001), dict(ds=float("nan")), dict(ds=float("inf")),
                    dict(ds=1e39), dict(step=1e-9)):
            assert call(**bad) == codes["UNSUPPORTED"], bad
        assert call(B=0, ds=0.0) == codes["OK"] and call(B=0, R=16, K=64) == codes["OK"]
        assert call(R=0, dims=(1025, 8, 8)) == codes["SHAPE"] and call(B=0, K=65) == codes["UNSUPPORTED"]   # the order of the checks
        for bad in (dict(field=None), dict(org=None), dict(L=None), dict(dirs=None), dict(result=None)):
            assert call(**bad) == codes["NULL"], bad
    pick = _lib.lib.regnet_grasp_retreat_pick
    assert _lib.PARAMS["regnet_grasp_retreat_pick"] == ["result", "B", "R", "best", "stream"]
    assert pick(fake, 0, 5, fake, None) == codes["OK"] and pick(None, 0, 16, None, None) == codes["OK"]
    assert pick(fake, -1, 5, fake, None) == codes["SHAPE"] and pick(fake, 1, 0, fake, None) == codes["SHAPE"]
    assert pick(fake, 1, 17, fake, None) == codes["UNSUPPORTED"] and pick(fake, 1 << 31, 5, fake, None) == codes["UNSUPPORTED"]
    assert pick(None, 1, 5, fake, None) == codes["NULL"] and pick(fake, 1, 5, None, None) == codes["NULL"]


def _status_codes():
    """REGNET_OK and the three error codes, read from the header's text."""
    import re
    from regnet_for_3d_grasping_amd import _lib
    with open(_lib.HEADER_PATH) as f:
        text = f.read()
    return {name: int(re.search(r"#define REGNET_%s \(?(-?\d+)\)?" % ("OK" if name == "OK" else "ERR_" + name), text).group(1))
            for name in ("OK", "NULL", "SHAPE", "UNSUPPORTED")}
