"""``GraspDetector(denoise=...)`` end to end: ``detect`` of a camera frame with the option is ``detect``, by a detector without it,
of the same cloud with the rows the numpy restatement (tests/outlier_reference.py) removes blanked on the host -- for an ``(xyz,
rgb)`` pair, a ``DepthFrame`` and a ``MultiView`` --, the one added key, the table plane estimated on the filtered cloud, the
untouched default, and the CLI flags.  The fixture is the one of tests/test_gpu_detect_fused.py."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from . import outlier_reference as ref
from .test_gpu_detect_fused import FUSE, SEED, _run, _same_state, parts  # noqa: F401  (the module-scoped fixture)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DENOISE = {"mode": "both", "radius": 0.03, "min_neighbours": 12, "knn": 8, "max_radius": 0.03, "std_ratio": 1.5}


_CACHE = {}


def _blanked(xyz, rgb, denoise, key):
    if (key, repr(denoise)) not in _CACHE:
        _CACHE[key, repr(denoise)] = _blank(xyz, rgb, denoise)
    return _CACHE[key, repr(denoise)]


def _blank(xyz, rgb, denoise):
    """The host pair with the rows the restatement removes at NaN / 0, and the restatement's histogram.  The statistical
    stage compares with the device's threshold where the two differ in the last bits (tests/test_gpu_outliers.py bounds them)."""
    from regnet_for_3d_grasping_amd import outliers
    p = outliers.OutlierParams.coerce(denoise)
    xyz, rgb = xyz.cpu().numpy(), rgb.cpu().numpy()
    thr = None
    if p.mode != "radius":
        thr = float(outliers.filter_cloud(torch.from_numpy(xyz).to(DEV), p).stats[3])
    want = ref.filter_cloud(xyz, p.mode, p.radius, p.min_neighbours, p.knn, p.max_radius, p.std_ratio, thr=thr)
    assert 0 < want["num"][ref.KEPT] and (p.mode == "radius" or want["num"][ref.KEPT] < ref.graph_rows(xyz).sum())
    return ref.apply(want["keep"], xyz, rgb), want["num"]


def _equal(got, want, keys):
    for key in keys:
        assert got[key].dtype == want[key].dtype and got[key].tobytes() == want[key].tobytes(), key


@pytest.mark.parametrize("kind", ["pair", "depth", "multiview"])
@pytest.mark.parametrize("denoise", [{}, DENOISE])
def test_detect_with_denoise_is_detect_of_the_blanked_cloud(parts, kind, denoise):  # noqa: F811
    from regnet_for_3d_grasping_amd import depth_frame, detect, outliers
    merged = parts[3]
    kw, added = {}, ()
    if kind == "pair":                                        # a host pair, as read_pcd gives it (float64)
        cloud = merged.xyz.double(), merged.rgb.double()
        frame = tuple(t.cpu().numpy() for t in cloud)
    elif kind == "depth":
        frame = parts[2].frames[0]
        cloud = depth_frame.to_cloud(frame, device=DEV)
    else:
        frame, cloud, kw, added = parts[2], merged.cloud(), {"fuse": FUSE}, detect.FUSE_KEYS
    (xyz, rgb), num = _blanked(cloud[0], cloud[1], denoise, kind)
    assert xyz.dtype == cloud[0].cpu().numpy().dtype
    got, got_state = _run(parts, frame, denoise=denoise, **kw)
    want, want_state = _run(parts, (xyz, rgb))
    assert tuple(want) == detect.RESULT_KEYS and tuple(got) == detect.RESULT_KEYS + added + detect.DENOISE_KEYS
    _equal(got, want, detect.RESULT_KEYS)
    assert _same_state(got_state, want_state) and len(got["points"]) > 1000
    assert got["denoise_num"].dtype == np.int32 and got["denoise_num"].shape == (5,) and np.array_equal(got["denoise_num"], num)
    device_num = outliers.filter_cloud(cloud[0], denoise).num
    assert np.array_equal(got["denoise_num"], device_num.cpu().numpy())
    plain, _ = _run(parts, frame, **kw)                       # the filter changed the record
    assert tuple(plain) == detect.RESULT_KEYS + added and len(plain["points"]) >= len(got["points"])
    assert not denoise or len(plain["points"]) > len(got["points"])


def test_the_plane_is_estimated_on_the_filtered_cloud(parts):  # noqa: F811
    from regnet_for_3d_grasping_amd import detect
    merged = parts[3]
    auto = {"range": (0.5, 1.2)}
    (xyz, rgb), _ = _blanked(merged.xyz, merged.rgb, DENOISE, "multiview")
    got, got_state = _run(parts, parts[2], fuse=FUSE, denoise=DENOISE, transform=auto)
    want, want_state = _run(parts, (xyz, rgb), transform=auto)
    assert tuple(got) == detect.RESULT_KEYS + detect.TABLE_KEYS + detect.FUSE_KEYS + detect.DENOISE_KEYS
    _equal(got, want, detect.RESULT_KEYS + detect.TABLE_KEYS)
    assert _same_state(got_state, want_state)
    unfiltered, _ = _run(parts, parts[2], fuse=FUSE, transform=auto)
    assert unfiltered["table_plane"].tobytes() != got["table_plane"].tobytes()


def test_records_and_frames_never_see_it(parts):  # noqa: F811
    from regnet_for_3d_grasping_amd import detect
    merged = parts[3]
    from regnet_for_3d_grasping_amd import np_random
    np.random.seed(SEED)
    with np_random.deferred():
        fr = detect.GraspDetector(parts[0], parts[1], denoise=DENOISE).ingest(merged.cloud())
        assert fr.denoised is not None and fr.denoised.num.shape == (5,)
        plain = detect.GraspDetector(parts[0], parts[1]).ingest(merged.cloud())
        remover = detect.GraspDetector(parts[0], parts[1], denoise={"radius": 0.001, "min_neighbours": 1000})
        assert plain.denoised is None and remover.ingest(plain) is plain         # (a filter that would remove every row)
    out, _ = _run(parts, plain, denoise={"radius": 0.001, "min_neighbours": 1000})
    assert tuple(out) == detect.RESULT_KEYS and len(out["points"]) > 1000


CHILD = """
import sys
import numpy as np, torch
from regnet_for_3d_grasping_amd import detect, pipeline, synthetic, ingest
score_net, region_net = pipeline.build_models("cuda:0")
scene = synthetic.make_batch(1000, 1, 25600)[0].numpy().astype(np.float64)
Tinv = np.linalg.inv(ingest.table_frame_transform())
frame = (scene[:, :3] @ Tinv[:3, :3].T + Tinv[:3, 3], np.rint(scene[:, 3:6] * 255.0) / 255.0)
np.random.seed(1)
out = detect.GraspDetector(score_net, region_net, bounds=(0.5, -0.5, 1.0, 0.5, -0.5)).detect(frame)
assert tuple(out) == detect.RESULT_KEYS, tuple(out)
assert "regnet_for_3d_grasping_amd.outliers" not in sys.modules
print("child ok")
"""


def test_without_denoise_the_module_is_not_imported():
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-c", CHILD], cwd=repo, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "child ok" in r.stdout, (r.stdout[-400:], r.stderr[-1200:])


def test_the_cli_flags_reach_outlier_params(parts):  # noqa: F811
    from regnet_for_3d_grasping_amd import detect, outliers
    parser = detect.build_parser()
    required = ["--folder", "x", "--load-score-path", "a", "--load-region-path", "b"]
    args = parser.parse_args(required + ["--outlier-mode", "both", "--outlier-radius", "0.03", "--outlier-min-neighbours", "12",
                                         "--outlier-knn", "8", "--outlier-max-radius", "0.03", "--outlier-std-ratio", "1.5"])
    detector = detect.GraspDetector(parts[0], parts[1], denoise=detect.outliers_from_args(args))
    assert detector.denoise == outliers.OutlierParams(**DENOISE)
    switch = detect.GraspDetector(parts[0], parts[1], denoise=detect.outliers_from_args(parser.parse_args(required + ["--denoise"])))
    assert switch.denoise == outliers.OutlierParams()
    assert detect.GraspDetector(parts[0], parts[1], denoise=detect.outliers_from_args(parser.parse_args(required))).denoise is None
    with pytest.raises(TypeError, match="denoise must be None"):
        detect.GraspDetector(parts[0], parts[1], denoise=3)
