"""Single-frame ingest: the front end of the reference's ``test.py`` (:101-129) without open3d and without a host pass
over the frame.

``read_pcd`` reads the depth-camera frame (PCD v0.7: ascii, binary, binary_compressed); ``ingest_frame`` moves it into the
table frame, crops it to the workspace, draws ``utils.noise_color``'s gains and the ``np.random.choice`` rows from numpy's
stream ON THE DEVICE and gathers the network's ``pc (1, N, 6)`` (csrc/ingest.hip + np_random's device draws);
``ingest_record`` is the ``real_data=False`` branch (:108-110) for a dataset record.  Everything after the upload is
asynchronous: the kept count stays in device memory and is read once, with the results (``Frame.download``).
"""
import pickle

import numpy as np

from . import _lib
from ._frame_util import MAX_FRAME_POINTS, require_cuda, to_device      # noqa: F401  (the limit is this module's too)

_call = _lib.call
_L = _lib.lib

NUM_POINTS = 25600                                   # test.py:61
DEFAULT_BOUNDS = (0.26, -0.4, 1.0, 0.65, 0.2)        # test.py:114-118: x < 0.26, x > -0.4, z < 1, y < 0.65, y > 0.2
CENTER_CAMERA = (0.0, 0.0, 1.658)                    # test.py:103

_PCD_KEYS = ("VERSION", "FIELDS", "SIZE", "TYPE", "COUNT", "WIDTH", "HEIGHT", "VIEWPOINT", "POINTS", "DATA")
_PCD_DTYPES = {("F", 4): "<f4", ("F", 8): "<f8", ("U", 1): "<u1", ("U", 2): "<u2", ("U", 4): "<u4", ("U", 8): "<u8",
               ("I", 1): "<i1", ("I", 2): "<i2", ("I", 4): "<i4", ("I", 8): "<i8"}


def lzf_decompress(data, size):
    """LZF-decompress ``data`` (bytes) into exactly ``size`` bytes (native host code, regnet_lzf_decompress)."""
    src = np.frombuffer(data, dtype=np.uint8)
    out = np.empty((int(size),), dtype=np.uint8)
    got = _L.regnet_lzf_decompress(src.ctypes.data if src.size else None, src.size, out.ctypes.data if out.size else None,
                                   out.size)
    if got < 0:
        raise ValueError("PCD: corrupt LZF stream (%s)" % _L.regnet_strerror(int(got)).decode())
    if got != size:
        raise ValueError("PCD: LZF stream holds %d bytes, the header promises %d" % (got, size))
    return out


def _pcd_header(raw):
    """-> (dict of header entries, offset of the body)."""
    meta, at = {}, 0
    while True:
        end = raw.find(b"\n", at)
        if end < 0:
            raise ValueError("PCD: header has no DATA line")
        line = raw[at:end].decode("ascii", errors="replace").strip()
        at = end + 1
        if not line or line.startswith("#"):
            continue
        parts = line.split()
        key = parts[0].upper()
        if key not in _PCD_KEYS:
            raise ValueError("PCD: unknown header entry %r" % parts[0])
        meta[key] = parts[1:]
        if key == "DATA":
            break
    for key in ("FIELDS", "SIZE", "TYPE", "WIDTH", "HEIGHT", "DATA"):
        if key not in meta:
            raise ValueError("PCD: header has no %s line" % key)
    return meta, at


def read_pcd(path):
    """Read a PCD v0.7 file -> ``(xyz float64 (M,3), rgb float64 (M,3) in [0,1], meta)`` -- what
    ``open3d.io.read_point_cloud`` gives test.py:102-106 as ``points`` / ``colors``.

    ``DATA ascii``, ``binary`` and ``binary_compressed``; ``x y z`` typed F4 or F8 (F4 values are widened exactly);
    the colour comes from a packed ``rgb`` / ``rgba`` field (F4-, U4- or I4-typed, PCL's 0x00RRGGBB packing) divided by
    255.0; other fields are skipped; organised frames (``HEIGHT > 1``) are flattened row-major; NaN rows are kept (the crop
    drops them).  A file WITHOUT a colour field is accepted and its colours are zero: open3d leaves ``colors`` empty there
    and the reference's ``np.c_[pc, pc_color]`` would fail, so there is no behaviour to match.
    ``meta``: ``fields, width, height, points, viewpoint, data, version``.  Malformed headers raise ``ValueError``."""
    with open(path, "rb") as f:
        raw = f.read()
    head, body_at = _pcd_header(raw)
    fields = head["FIELDS"]
    try:
        sizes = [int(v) for v in head["SIZE"]]
        counts = [int(v) for v in head.get("COUNT", ["1"] * len(fields))]
        width, height = int(head["WIDTH"][0]), int(head["HEIGHT"][0])
        points = int(head["POINTS"][0]) if "POINTS" in head else width * height
    except (ValueError, IndexError):
        raise ValueError("PCD: non-numeric SIZE / COUNT / WIDTH / HEIGHT / POINTS")
    types = [t.upper() for t in head["TYPE"]]
    if not (len(fields) == len(sizes) == len(types) == len(counts)) or not fields:
        raise ValueError("PCD: FIELDS, SIZE, TYPE and COUNT disagree in length")
    if width < 0 or height < 0 or points != width * height:
        raise ValueError("PCD: POINTS %d is not WIDTH x HEIGHT = %d x %d" % (points, width, height))
    if any(c < 1 for c in counts):
        raise ValueError("PCD: COUNT entries must be at least 1")
    kinds = []
    for t, s in zip(types, sizes):
        if (t, s) not in _PCD_DTYPES:
            raise ValueError("PCD: unsupported field type %s%d" % (t, s))
        kinds.append(_PCD_DTYPES[(t, s)])
    for name in ("x", "y", "z"):
        if fields.count(name) != 1 or counts[fields.index(name)] != 1 or types[fields.index(name)] != "F":
            raise ValueError("PCD: one floating-point %r field is required" % name)
    mode = head["DATA"][0].lower() if head["DATA"] else ""
    body = raw[body_at:]
    dtype = np.dtype([("f%d" % i, kinds[i], (counts[i],)) for i in range(len(fields))])
    if mode == "ascii":
        tokens = body.split()
        per_row = sum(counts)
        if len(tokens) < points * per_row:
            raise ValueError("PCD: ascii body holds %d values, %d expected" % (len(tokens), points * per_row))
        table = np.array(tokens[:points * per_row], dtype=bytes).reshape(points, per_row)
        columns, col = {}, 0
        for i, kind in enumerate(kinds):
            text = np.char.decode(table[:, col:col + counts[i]], "ascii")
            try:        # floats through numpy's decimal parser, integers through Python ints (exact for U4 / U8)
                columns[i] = text.astype(kind) if kind[1] == "f" else np.array([[int(v) for v in row] for row in text]).astype(kind)
            except (ValueError, OverflowError):
                raise ValueError("PCD: ascii field %r holds a value that is not a %s%d" % (fields[i], types[i], sizes[i]))
            col += counts[i]
    elif mode == "binary":
        if len(body) < points * dtype.itemsize:
            raise ValueError("PCD: binary body holds %d bytes, %d expected" % (len(body), points * dtype.itemsize))
        rec = np.frombuffer(body, dtype=dtype, count=points)
        columns = {i: rec["f%d" % i] for i in range(len(fields))}
    elif mode == "binary_compressed":
        if len(body) < 8:
            raise ValueError("PCD: binary_compressed body has no size words")
        packed, unpacked = (int(v) for v in np.frombuffer(body[:8], dtype="<u4"))
        if unpacked != points * dtype.itemsize or len(body) < 8 + packed:
            raise ValueError("PCD: binary_compressed sizes do not match the header")
        flat = lzf_decompress(body[8:8 + packed], unpacked)
        columns, at = {}, 0                      # fields are stored one after the other (structure of arrays)
        for i, kind in enumerate(kinds):
            n = points * counts[i] * sizes[i]
            columns[i] = np.frombuffer(flat[at:at + n].tobytes(), dtype=kind).reshape(points, counts[i])
            at += n
    else:
        raise ValueError("PCD: unknown DATA mode %r" % mode)
    xyz = np.stack([np.asarray(columns[fields.index(n)]).reshape(points).astype(np.float64) for n in ("x", "y", "z")], axis=1)
    rgb = np.zeros((points, 3), dtype=np.float64)
    for name in ("rgb", "rgba"):
        if name in fields:
            i = fields.index(name)
            if sizes[i] != 4 or counts[i] != 1:
                raise ValueError("PCD: the %s field must be one 4-byte value" % name)
            word = np.ascontiguousarray(np.asarray(columns[i]).reshape(points)).view(np.uint32)
            rgb = np.stack([(word >> 16) & 255, (word >> 8) & 255, word & 255], axis=1).astype(np.float64) / 255.0
            break
    meta = {"fields": list(fields), "width": width, "height": height, "points": points, "data": mode,
            "viewpoint": [float(v) for v in head.get("VIEWPOINT", ["0", "0", "0", "1", "0", "0", "0"])],
            "version": (head.get("VERSION") or [""])[0]}
    return np.ascontiguousarray(xyz), np.ascontiguousarray(rgb), meta


def table_frame_transform(center_camera=CENTER_CAMERA):
    """``utils.local_to_global_transformation_quat`` (utils.py:433-440) in float64: the rotation
    ``quat2mat(euler2quat(-0.87 pi, 0, 0))`` (static ``sxyz`` axes) and the translation ``center_camera``.

    RESTATED from the formulas transforms3d publishes (``euler2quat``: half-angle products; ``quat2mat``: the
    ``2 / |q|^2``-scaled products) and NOT pinned against the library, which this package does not depend on; that is why
    every consumer takes the transform as an argument and this is only the default."""
    ai, aj, ak = -0.87 * np.pi / 2.0, 0.0, 0.0               # euler2quat halves the angles first
    ci, si, cj, sj, ck, sk = np.cos(ai), np.sin(ai), np.cos(aj), np.sin(aj), np.cos(ak), np.sin(ak)
    cc, cs, sc, ss = ci * ck, ci * sk, si * ck, si * sk
    w, x, y, z = cj * cc + sj * ss, cj * sc - sj * cs, cj * ss + sj * cc, cj * cs - sj * sc   # (w, x, y, z), static xyz
    s = 2.0 / (w * w + x * x + y * y + z * z)                # quat2mat
    X, Y, Z = x * s, y * s, z * s
    wX, wY, wZ, xX, xY, xZ, yY, yZ, zZ = w * X, w * Y, w * Z, x * X, x * Y, x * Z, y * Y, y * Z, z * Z
    T = np.eye(4)
    T[0:3, 0:3] = [[1.0 - (yY + zZ), xY - wZ, xZ + wY], [xY + wZ, 1.0 - (xX + zZ), yZ - wX], [xZ - wY, yZ + wX, 1.0 - (xX + yY)]]
    T[0:3, 3] = np.asarray(center_camera, dtype=np.float64)
    return T


class Frame:
    """What test.py holds after :129.  ``pc`` (1, N, 6) float32 on the device; ``points_back`` / ``colors_back`` (rows, 3):
    the cropped, un-jittered cloud (``pc_back`` / ``color_back`` of :119) in device buffers of the INPUT's row count whose
    first ``count`` rows are valid; ``count`` (1,) int32 on the device; ``points32`` the float32 coordinates
    (``torch.Tensor(pc_back)``) the collision filter takes.  ``download()`` is the one blocking read."""

    def __init__(self, pc, points_back, colors_back, points32, count, out_of_range, source=None):
        self.pc, self.points_back, self.colors_back, self.points32 = pc, points_back, colors_back, points32
        self.count, self.out_of_range, self.source = count, out_of_range, source
        self.fused = self.table = None           # GraspDetector.ingest: the fusion.Fused / the (transform, plane) it found

    def kept(self):
        """The number of kept rows as a Python int (a 4-byte blocking read).  Raises ``ValueError`` when nothing was kept:
        ``np.random.choice(0, N)`` raises in the reference."""
        import torch
        n, bad = (int(v) for v in torch.cat((self.count, self.out_of_range)).cpu())
        if n == 0:
            raise ValueError("ingest: no point of the frame lies inside the workspace bounds")
        if bad:
            raise RuntimeError("ingest: a drawn row lies outside the kept list")
        return n

    def download(self, kept=None):
        """-> (points_back (count,3), colors_back (count,3)) numpy arrays of the dtypes the reference pickles: float64 for a
        camera frame, float32 for a dataset record."""
        n = self.kept() if kept is None else int(kept)
        return self.points_back[:n].cpu().numpy(), self.colors_back[:n].cpu().numpy()


def crop_frame(xyz, rgb, transform, bounds=DEFAULT_BOUNDS, drop_nonfinite=True, with_source=False):
    """regnet_ingest_crop_*: ``xyz`` / ``rgb`` (M,3) contiguous GPU tensors of one dtype (float32 or float64) ->
    ``(kept_xyz64 (M,3), kept_xyz32 (M,3), kept_rgb (M,3) float64, count (1,) int32, source (M,) int32 or None)``, all on
    the device; the first ``count`` rows are the kept points in input order.  No synchronisation."""
    import torch
    T = np.ascontiguousarray(transform, dtype=np.float64)
    if T.shape != (4, 4):
        raise ValueError("transform must be 4x4")
    b = np.ascontiguousarray(bounds, dtype=np.float64)
    if b.shape != (5,):
        raise ValueError("bounds must be (x_hi, x_lo, z_hi, y_hi, y_lo)")
    xyz = require_cuda("crop_frame: xyz", xyz, (torch.float32, torch.float64), 3).contiguous()
    rgb = require_cuda("crop_frame: rgb", rgb, xyz.dtype, 3).contiguous()
    if rgb.shape[0] != xyz.shape[0]:
        raise ValueError("xyz and rgb must both be (M, 3)")
    M, dev = int(xyz.shape[0]), xyz.device
    if M > MAX_FRAME_POINTS:
        raise ValueError("frames of more than 2^21 points are not supported")
    kept64 = torch.empty((M, 3), dtype=torch.float64, device=dev)
    kept32 = torch.empty((M, 3), dtype=torch.float32, device=dev)
    kept_rgb = torch.empty((M, 3), dtype=torch.float64, device=dev)
    source = torch.empty((M,), dtype=torch.int32, device=dev) if with_source else None
    count = torch.empty((1,), dtype=torch.int32, device=dev)
    ws = torch.empty((max(int(_L.regnet_ingest_crop_workspace_bytes(M)), 8),), dtype=torch.uint8, device=dev)
    _call("regnet_ingest_crop_f64" if xyz.dtype == torch.float64 else "regnet_ingest_crop_f32", xyz, xyz.data_ptr(),
          rgb.data_ptr(), M, T.ctypes.data, b.ctypes.data, 1 if drop_nonfinite else 0, kept64.data_ptr(), kept32.data_ptr(),
          kept_rgb.data_ptr(), source.data_ptr() if with_source else None, count.data_ptr(), ws.data_ptr())
    return kept64, kept32, kept_rgb, count, source


def _resample(xyz32, rgb, count, num_points):
    """noise_color's three draws, the choice of ``num_points`` rows (mode 0 = test.py:123-126), the gather -> (pc, flag)."""
    import torch
    from . import np_random
    M, N, dev = int(xyz32.shape[0]), int(num_points), xyz32.device
    bad = torch.zeros((1,), dtype=torch.int32, device=dev)
    rand3 = np_random.rand_device(3, dev)                                    # utils.noise_color draws first
    pick = np_random.choice_rows_device(count, N, 0, max(M, 1))[0].view(N)
    pc = torch.empty((N, 6), dtype=torch.float32, device=dev)
    _call("regnet_ingest_resample_f32", xyz32, xyz32.data_ptr(), rgb.data_ptr(), 1 if rgb.dtype == torch.float64 else 0,
          count.data_ptr(), M, pick.data_ptr(), N, rand3.data_ptr(), pc.data_ptr(), bad.data_ptr())
    return pc.view(1, N, 6), bad


def ingest_frame(xyz, rgb, transform=None, bounds=DEFAULT_BOUNDS, num_points=NUM_POINTS, device="cuda:0", drop_nonfinite=True,
                 with_source=False):
    """test.py:104-129 for one camera frame -> ``Frame``.

    ``xyz`` / ``rgb`` (M,3): numpy arrays or tensors, float64 (what ``read_pcd`` returns) or float32, both of one dtype; host
    arrays go up once through ``host_io``, device tensors are used where they are.  ``transform``: row-major 4x4 float64
    (default ``table_frame_transform()``); ``bounds = (x_hi, x_lo, z_hi, y_hi, y_lo)``, all strict.  ``drop_nonfinite``
    drops rows with a NaN / infinite coordinate before the tests (an explicit guard: they fail the two-sided tests anyway).  numpy's global generator is
    consumed exactly as the reference does: ``rand(3)`` (noise_color), then ``choice(count, num_points)`` without
    replacement when ``count >= num_points``, else with.  No host synchronisation when the frame is already on the device
    and the generator state is (a freshly seeded host generator is handed over with one small blocking upload); as after
    ``ScoreDataset.gpu_item``, call ``np_random.flush()`` or leave a ``np_random.deferred()`` block before using
    ``np.random`` on the host again."""
    import torch
    dev = torch.device(device)
    xyz_d, rgb_d = to_device(xyz, dev), to_device(rgb, dev)
    kept64, kept32, kept_rgb, count, source = crop_frame(xyz_d, rgb_d, table_frame_transform() if transform is None else transform,
                                                         bounds, drop_nonfinite, with_source)
    pc, bad = _resample(kept32, kept_rgb, count, num_points)
    return Frame(pc, kept64, kept_rgb, kept32, count, bad, source)


def ingest_record(path_or_dict, num_points=NUM_POINTS, device="cuda:0"):
    """The ``real_data=False`` branch (test.py:108-110, :119-129) for a dataset record (a ``.p`` path or its dict):
    ``view_cloud`` / ``view_cloud_color`` as float32, no transform, no crop -> ``Frame`` (``points_back`` float32)."""
    import torch
    data = path_or_dict
    if not isinstance(data, dict):
        with open(path_or_dict, "rb") as f:
            data = pickle.load(f)
    dev = torch.device(device)
    cloud = to_device(np.asarray(data["view_cloud"]).astype(np.float32), dev)
    color = to_device(np.asarray(data["view_cloud_color"]).astype(np.float32), dev)
    if cloud.dim() != 2 or cloud.shape[1] != 3 or tuple(color.shape) != tuple(cloud.shape):
        raise ValueError("view_cloud and view_cloud_color must both be (M, 3)")
    count = torch.full((1,), int(cloud.shape[0]), dtype=torch.int32, device=cloud.device)
    pc, bad = _resample(cloud, color, count, num_points)
    return Frame(pc, cloud, color, cloud, count, bad)
