"""``_lib.call`` on the device: the appended stream is torch's current one, an explicit handle overrides it, an entry point
without a stream parameter gets nothing appended, and a failed launch names its entry point."""
import pytest
import torch

pytestmark = pytest.mark.gpu

B, N, M = 2, 64, 8


@pytest.fixture(scope="module")
def cloud():
    from regnet_for_3d_grasping_amd import pn2_ext
    g = torch.Generator().manual_seed(11)
    xyz = torch.rand((B, 3, N), generator=g).cuda()
    want = pn2_ext.farthest_point_sample(xyz, M)
    torch.cuda.synchronize()
    return xyz, want.cpu()


def _fps(xyz, index, **kw):
    from regnet_for_3d_grasping_amd import _lib
    assert _lib.lib.regnet_fps_workspace_bytes(B, N, M) == 0        # register-resident kernel: no workspace to hand in
    return _lib.call("regnet_fps_f32", xyz, xyz.data_ptr(), *xyz.stride(), B, N, M, index.data_ptr(), None, **kw)


def test_the_appended_stream_is_the_current_one(cloud):
    xyz, want = cloud
    s = torch.cuda.Stream()
    index = torch.full((B, M), -1, dtype=torch.int64, device=xyz.device)
    torch.cuda.synchronize()            # xyz and the fill are done: from here on only `s` is waited for
    with torch.cuda.stream(s):
        assert _fps(xyz, index) == 0
    s.synchronize()
    assert torch.equal(index.cpu(), want)


def test_an_explicit_stream_handle(cloud):
    xyz, want = cloud
    other = torch.cuda.Stream()
    index = torch.full((B, M), -1, dtype=torch.int64, device=xyz.device)
    ready = torch.cuda.Event()
    ready.record(torch.cuda.current_stream())
    other.wait_event(ready)             # the fill above is ordered before the launch on `other`
    assert _fps(xyz, index, stream=other.cuda_stream) == 0
    other.synchronize()
    assert torch.equal(index.cpu(), want)


def test_a_query_has_nothing_appended(cloud):
    from regnet_for_3d_grasping_amd import _lib
    xyz, _ = cloud
    assert not _lib.HAS_STREAM["regnet_fps_workspace_bytes"]
    assert len(_lib.SIGNATURES["regnet_fps_workspace_bytes"][1]) == 3
    for shape in ((B, N, M), (4, 5120, 1024)):
        assert _lib.call("regnet_fps_workspace_bytes", xyz, *shape) == _lib.lib.regnet_fps_workspace_bytes(*shape)
    assert _lib.call("regnet_fps_workspace_bytes", xyz, 4, 5120, 1024) == 4 * 5120 * 4


def test_a_shape_error_names_the_entry_point(cloud):
    from regnet_for_3d_grasping_amd import _lib
    xyz, _ = cloud
    index = torch.empty((B, 1), dtype=torch.int64, device=xyz.device)
    with pytest.raises(RuntimeError, match="regnet_fps_f32 failed: shape"):
        _lib.call("regnet_fps_f32", xyz, xyz.data_ptr(), *xyz.stride(), B, N, 0, index.data_ptr(), None)    # M = 0
