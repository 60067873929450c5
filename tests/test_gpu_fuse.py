"""Multi-view fusion on the device (csrc/fuse.hip, fusion.py) against the numpy restatement of its contract
(tests/fuse_reference.py): the integer outputs equal, ``xyz`` / ``rgb`` byte for byte, the rows beyond ``K`` at their sentinels
(the restatement's arrays are ``max_voxels`` rows long, so whole-array equality covers them); every case runs twice and gives the
same bytes."""
import numpy as np
import pytest
import torch

from . import depth_reference
from . import fuse_reference as ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
f32 = np.float32
KEYS = ("xyz", "rgb", "count", "views", "first", "num")


def _up(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DEV)


def _device(clouds, poses=None, params=None, **kw):
    from regnet_for_3d_grasping_amd import fusion
    fused = fusion.voxel_merge([(_up(xyz), _up(rgb)) for xyz, rgb in clouds], poses, params, **kw)
    torch.cuda.synchronize()
    return {key: getattr(fused, key).cpu().numpy() for key in KEYS}, fused


def _equal(got, want, keys=KEYS):
    for key in keys:
        assert got[key].dtype == want[key].dtype and got[key].shape == want[key].shape, key
        if key in ("xyz", "rgb"):
            assert got[key].tobytes() == want[key].tobytes(), key
        else:
            assert np.array_equal(got[key], want[key]), (key, got[key][:8], want[key][:8])


def _check(clouds, poses=None, **params):
    params.setdefault("max_voxels", 512)
    want = ref.merge(clouds, poses, params)
    assert want["num"][3] == 0
    got, fused = _device(clouds, poses, params)
    again, _ = _device(clouds, poses, params)
    _equal(got, want)
    _equal(again, got)                                # the order of the atomics does not show
    assert fused.check() == tuple(int(v) for v in want["num"][:3])
    K = want["K"]
    assert np.isnan(got["xyz"][K:]).all() and (got["xyz"][K:].view(np.uint32) == 0x7FC00000).all()
    assert (got["rgb"][K:] == 0).all() and (got["count"][K:] == -1).all() and (got["first"][K:] == -1).all()
    return got, want


def _cloud(seed, n, extent=0.1, centre=0.0):
    rng = np.random.RandomState(seed)
    return (rng.uniform(centre - extent, centre + extent, (n, 3)).astype(np.float32), rng.uniform(0, 1, (n, 3)).astype(np.float32))


def _pose(seed):
    rng = np.random.RandomState(seed)
    q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    T = np.eye(4)
    T[:3, :3] = q * np.sign(np.linalg.det(q))
    T[:3, 3] = rng.uniform(-0.05, 0.05, 3)
    return T


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 257])
def test_row_counts(n):
    got, want = _check([_cloud(n, n)], [_pose(1)], voxel=0.05)
    assert want["num"][1] == n and (n < 63 or (want["count"] > 1).any())
    if n == 0:
        assert got["num"].tolist() == [0, 0, 0, 0]


@pytest.mark.parametrize("rows", [[300], [129, 200], [100, 0, 65, 1, 300, 64, 7, 129], [0, 0]])
def test_views_with_ragged_row_counts(rows):
    clouds = [_cloud(10 + v, n) for v, n in enumerate(rows)]
    poses = [None] + [_pose(20 + v) for v in range(1, len(rows))]
    got, want = _check(clouds, poses, voxel=0.04, origin=(0.01, -0.02, 0.003))
    seen = np.bitwise_or.reduce(want["views"][:want["K"]]) if want["K"] else 0
    assert seen == sum(1 << v for v, n in enumerate(rows) if n)
    assert len(rows) == 1 or sum(rows) == 0 or (want["views"][:want["K"]] & (want["views"][:want["K"]] - 1)).any()   # shared voxels
    from regnet_for_3d_grasping_amd import fusion
    fused = fusion.voxel_merge([(_up(x), _up(c)) for x, c in clouds], poses, {"voxel": 0.04, "origin": (0.01, -0.02, 0.003),
                                                                               "max_voxels": 512})
    per_view = [int(((want["views"][:want["K"]] >> v) & 1).sum()) for v in range(len(rows))]
    assert fused.per_view().tolist() == per_view
    xyz, rgb = fused.cloud()
    assert xyz is fused.xyz and rgb is fused.rgb
    colourless, _ = _device([(x, None) for x, _ in clouds], poses, {"voxel": 0.04, "origin": (0.01, -0.02, 0.003), "max_voxels": 512})
    _equal(colourless, ref.merge([(x, None) for x, _ in clouds], poses, {"voxel": 0.04, "origin": (0.01, -0.02, 0.003),
                                                                         "max_voxels": 512}))
    assert (colourless["rgb"] == 0).all() and colourless["xyz"].tobytes() == got["xyz"].tobytes()


def test_a_voxel_below_the_spacing_is_a_transform_and_sort():
    xyz, rgb = _cloud(3, 1000, extent=1.0)
    rgb = rgb * f32(1.4) - f32(0.2)                  # colours outside [0, 1] pass unchanged
    pose = _pose(4)
    got, want = _check([(xyz, rgb)], [pose], voxel=1e-5, max_voxels=1024)
    assert want["K"] == 1000 and (got["count"][:1000] == 1).all()
    moved, i, _, _, inside = ref.voxel_coords(xyz, ref.pose12(pose), np.zeros(3, dtype=np.float32), ref.inverse_voxel(1e-5))
    assert inside.all()
    order = np.argsort(np.array([ref.key_of(v) for v in i], dtype=np.int64))
    assert np.array_equal(got["first"][:1000], order)
    assert got["xyz"][:1000].tobytes() == moved[order].tobytes() and got["rgb"][:1000].tobytes() == rgb[order].tobytes()


@pytest.mark.parametrize("voxel", [0.25, 0.002])
def test_points_on_voxel_faces_and_one_ulp_either_side(voxel):
    faces = (np.arange(-6, 7, dtype=np.float64) * voxel).astype(np.float32)
    values = np.concatenate([faces, np.nextafter(faces, f32(np.inf)), np.nextafter(faces, f32(-np.inf)),
                             np.array([0.0, -0.0, 1e-30, -1e-30], dtype=np.float32)])
    pts = np.zeros((3 * len(values), 3), dtype=np.float32)
    for axis in range(3):
        pts[axis * len(values):(axis + 1) * len(values), axis] = values
    pts = np.concatenate([pts, pts + f32(voxel / 4)])
    got, want = _check([(pts, None)], voxel=voxel)
    assert want["num"][1] == len(pts) and want["K"] > 30
    shifted, _ = _check([(pts, None)], voxel=voxel, origin=(voxel / 2, -voxel / 2, voxel / 3))
    assert shifted["num"][0] != got["num"][0] or shifted["xyz"].tobytes() != got["xyz"].tobytes()


def test_contention_on_one_voxel_and_on_a_voxel_per_wave():
    rng = np.random.RandomState(8)
    one = (rng.uniform(0.0, 0.0099, (4096, 3)).astype(np.float32), rng.uniform(0, 1, (4096, 3)).astype(np.float32))
    got, want = _check([one], voxel=0.01)
    assert want["K"] == 1 and got["count"][0] == 4096 and got["first"][0] == 0
    cells = np.repeat(np.arange(64), 64)              # a wave's 64 lanes share a voxel
    xyz = (rng.uniform(0.0, 0.0099, (4096, 3)) + np.stack([cells % 4, (cells // 4) % 4, cells // 16], axis=1) * 0.01)
    xyz = (xyz - 0.02).astype(np.float32)
    rgb = rng.uniform(0, 1, (4096, 3)).astype(np.float32)
    grouped, want = _check([(xyz, rgb)], voxel=0.01)
    assert want["K"] >= 64 and want["count"][:want["K"]].sum() == 4096 and want["count"].max() >= 60
    perm = np.arange(4096).reshape(64, 64).T.reshape(-1)          # row j holds voxel j % 64: every lane its own voxel
    spread, _ = _check([(xyz[perm], rgb[perm])], voxel=0.01)
    for key in ("xyz", "rgb", "count", "views"):
        assert spread[key].tobytes() == grouped[key].tobytes(), key


def test_forty_keys_sharing_a_home_slot_wrap_around_the_table():
    slots, inv, zero = 128, ref.inverse_voxel(1.0), np.zeros(3, dtype=np.float32)
    assert ref.table_slots(64) == slots
    cells = [(x, y) for x in range(-60, 60) for y in range(-60, 60)
             if ref.home_slot(ref.key_of((x, y, 0)), slots) == 120][:40]
    assert len(cells) == 40
    pts = np.array([[x + 0.5, y + 0.25, 0.75] for x, y in cells] * 2, dtype=np.float32)
    pts[40:, 2] = 0.25
    assert all(ref.key(*p, ref.pose12(None), zero, inv) == ref.key_of((x, y, 0)) for p, (x, y) in zip(pts, cells))
    got, want = _check([(pts, None)], voxel=1.0, max_voxels=64)
    assert want["K"] == 40 and (got["count"][:40] == 2).all() and (got["xyz"][:40, 2] == 0.5).all()


@pytest.mark.parametrize("voxels,overflow", [(63, 0), (64, 0), (65, 1)])
def test_capacity_and_guarded_outputs(voxels, overflow):
    from regnet_for_3d_grasping_amd import fusion
    rng = np.random.RandomState(voxels)
    cells = rng.permutation(512)[:voxels]
    xyz = (np.stack([cells % 8, (cells // 8) % 8, cells // 64], axis=1) + 0.5).astype(np.float32)
    xyz = np.concatenate([xyz, xyz[::2] + f32(0.25)])
    rgb = rng.uniform(0, 1, xyz.shape).astype(np.float32)
    params = {"voxel": 1.0, "max_voxels": 64}
    want = ref.merge([(xyz, rgb)], None, params)
    assert want["num"][3] == overflow
    guard, mv = 64, 64
    shapes = ((mv * 3, torch.float32), (mv * 3, torch.float32), (mv, torch.int32), (mv, torch.int32), (mv, torch.int32),
              (4, torch.int32))
    padded = [torch.full((guard + n + guard,), 77, dtype=dtype, device=DEV) for n, dtype in shapes]
    out = tuple(p[guard:guard + n].view(-1, 3) if i < 2 else p[guard:guard + n] for i, (p, (n, _)) in enumerate(zip(padded, shapes)))
    fused = fusion.voxel_merge([(_up(xyz), _up(rgb))], None, params, out=out)
    torch.cuda.synchronize()
    assert fused.xyz.data_ptr() == out[0].data_ptr()
    for p, (n, _) in zip(padded, shapes):
        assert (p[:guard] == 77).all() and (p[guard + n:] == 77).all()
    assert int(fused.num[3]) == overflow
    if overflow:
        with pytest.raises(ValueError, match="max_voxels = 64"):
            fused.check()
    else:
        _equal({key: getattr(fused, key).cpu().numpy() for key in KEYS}, want)
        assert fused.check() == (voxels, len(xyz), 0)


def test_dropped_rows_are_counted():
    xyz, rgb = _cloud(12, 600)
    kind = np.random.RandomState(13).rand(600)
    xyz[kind < 0.1] = np.nan
    xyz[(kind > 0.1) & (kind < 0.15), 1] = np.inf
    xyz[(kind > 0.15) & (kind < 0.2), 2] = -np.inf
    xyz[(kind > 0.2) & (kind < 0.25), 0] = f32(0.05 * 2 ** 20)           # i = 2^20: the first one out of range
    xyz[(kind > 0.25) & (kind < 0.3), 1] = f32(-0.05 * (2 ** 20 + 1))    # i = -2^20 - 1
    xyz[(kind > 0.3) & (kind < 0.35), 2] = f32(3e38)
    xyz[(kind > 0.35) & (kind < 0.4), 0] = f32(0.05 * (2 ** 20 - 1))     # i = 2^20 - 1: the last one in range
    xyz[(kind > 0.4) & (kind < 0.45), 1] = f32(-0.05 * 2 ** 20 + 0.01)   # i = -2^20: the first one in range
    rgb[kind > 0.9] = np.nan                                             # a NaN colour counts as 0
    got, want = _check([(xyz, rgb), (xyz[:100], rgb[:100])], [None, _pose(2)], voxel=0.05)
    assert want["num"][2] >= int((kind < 0.35).sum()) > 150 and want["num"][1] + want["num"][2] == 700
    assert want["num"][1] >= int(((kind > 0.35) & (kind < 0.45)).sum()) > 30


@pytest.mark.parametrize("min_count", [2, 5])
def test_min_count(min_count):
    clouds = [_cloud(30, 400), _cloud(31, 300)]
    full, _ = _check(clouds, [None, _pose(5)], voxel=0.04)
    got, want = _check(clouds, [None, _pose(5)], voxel=0.04, min_count=min_count)
    assert 0 < want["K"] < full["num"][0] and (got["count"][:want["K"]] >= min_count).all()
    assert want["K"] == int((full["count"] >= min_count).sum()) and np.array_equal(got["num"][1:], full["num"][1:])


def test_the_order_of_the_rows_does_not_show():
    xyz, rgb = _cloud(40, 2000)
    got, _ = _check([(xyz, rgb)], [_pose(6)], voxel=0.03)
    perm = np.random.RandomState(41).permutation(2000)
    shuffled, _ = _check([(xyz[perm], rgb[perm])], [_pose(6)], voxel=0.03)
    for key in ("xyz", "rgb", "count", "views", "num"):
        assert shuffled[key].tobytes() == got[key].tobytes(), key
    K = got["num"][0]
    _, i, _, _, _ = ref.voxel_coords(xyz, ref.pose12(_pose(6)), np.zeros(3, dtype=np.float32), ref.inverse_voxel(0.03))
    row_key = np.array([ref.key_of(v) for v in i], dtype=np.int64)
    assert np.array_equal(row_key[perm[shuffled["first"][:K]]], row_key[got["first"][:K]])
    inverse = np.argsort(perm)                        # original row -> shuffled row: first is the voxel's smallest shuffled row
    members = {}
    for row, key in enumerate(row_key):
        members.setdefault(key, []).append(inverse[row])
    assert [min(members[k]) for k in row_key[got["first"][:K]]] == shuffled["first"][:K].tolist()


def test_a_side_stream():
    clouds = [_cloud(50, 500), _cloud(51, 257)]
    poses = [None, _pose(7)]
    params = {"voxel": 0.04, "max_voxels": 512}
    want = ref.merge(clouds, poses, params)
    stream = torch.cuda.Stream(device=DEV)
    got, _ = _device(clouds, poses, params, stream=stream)
    _equal(got, want)


def test_two_views_of_one_scene():
    from regnet_for_3d_grasping_amd import depth_frame, fusion
    frames, poses = ref.two_view_scene()
    clouds = [depth_reference.to_cloud(**kw)[:2] for kw in frames]
    params = {"voxel": ref.TWO_VIEW_VOXEL, "max_voxels": 4096}
    want = ref.merge(clouds, poses, params)
    assert want["K"] == ref.TWO_VIEW_K
    mv = fusion.MultiView([depth_frame.DepthFrame(**kw) for kw in frames], poses)
    fused = fusion.fuse_frames(mv, None, params, device=DEV)
    torch.cuda.synchronize()
    got = {key: getattr(fused, key).cpu().numpy() for key in KEYS}
    _equal(got, want)
    K = got["num"][0]
    assert K == ref.TWO_VIEW_K and (got["views"][:K] == 3).sum() == (want["views"][:K] == 3).sum() > 50
    assert fused.per_view().tolist() == [int(((want["views"][:K] >> v) & 1).sum()) for v in range(2)]


def test_refusals():
    from regnet_for_3d_grasping_amd import fusion
    cloud = (_up(np.zeros((4, 3))), _up(np.zeros((4, 3))))
    with pytest.raises(RuntimeError, match="no CPU path"):
        fusion.voxel_merge([(cloud[0].cpu(), cloud[1])])
    with pytest.raises(TypeError):
        fusion.voxel_merge([(cloud[0].double(), cloud[1])])
    with pytest.raises(ValueError):
        fusion.voxel_merge([cloud, (cloud[0], None)])
    with pytest.raises(ValueError):
        fusion.voxel_merge([cloud] * 9)
    with pytest.raises(ValueError):
        fusion.voxel_merge([cloud], params={"voxel": 0.0})
