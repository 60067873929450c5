"""numpy restatement of the reference's single-file front end (test.py:112-127 + utils.noise_color, utils.py:426-431) and
the seeded inputs the ingest tests and tests/golden/make_golden_ingest.py share.  Checker only: nothing here is imported by
the package."""
import numpy as np

ALL_POINTS_NUM = 25600
DEFAULT_BOUNDS = (0.26, -0.4, 1.0, 0.65, 0.2)      # x_hi, x_lo, z_hi, y_hi, y_lo


def transform_points(xyz, T):
    """The 4x4 times (x, y, z, 1) product with every product and sum rounded on its own, left to right."""
    x, y, z = (np.asarray(xyz[:, k], dtype=np.float64) for k in range(3))
    T = np.asarray(T, dtype=np.float64)
    return np.stack([((T[r, 0] * x + T[r, 1] * y) + T[r, 2] * z) + T[r, 3] for r in range(3)], axis=1)


def crop(xyz, rgb, T, bounds=DEFAULT_BOUNDS, drop_nonfinite=True):
    """test.py:104-119 on arrays -> (pc (K,6) float64, source rows (K,))."""
    src = np.arange(len(xyz))
    with np.errstate(invalid="ignore"):
        if drop_nonfinite:
            src = src[np.isfinite(np.asarray(xyz, dtype=np.float64)).all(axis=1)]
        pc = np.c_[transform_points(np.asarray(xyz)[src], T), np.asarray(rgb, dtype=np.float64)[src]]
        x_hi, x_lo, z_hi, y_hi, y_lo = bounds
        for col, hi, bound in ((0, True, x_hi), (0, False, x_lo), (2, True, z_hi), (1, True, y_hi), (1, False, y_lo)):
            keep = pc[:, col] < bound if hi else pc[:, col] > bound     # the literal five masks of :114-118, in order
            pc, src = pc[keep], src[keep]
    return pc, src


def noise_color(pc):
    """utils.noise_color (utils.py:426-431), in place like the reference."""
    obj_color_time = 1 - np.random.rand(3) / 5
    for i in range(3, 6):
        pc[:, i] *= obj_color_time[i - 3]
    return pc


def resample(pc, all_points_num=ALL_POINTS_NUM):
    """test.py:119-129 -> (pc (N,6) float32 as torch.Tensor(pc) rounds it, pc_back, color_back)."""
    pc_back, color_back = pc[:, :3].copy(), pc[:, 3:6].copy()
    pc = noise_color(pc)
    if len(pc) >= all_points_num:
        select = np.random.choice(len(pc), all_points_num, replace=False)
    else:
        select = np.random.choice(len(pc), all_points_num, replace=True)
    return pc[select].astype(np.float32), pc_back, color_back


def record_cloud(seed, num_points):
    """A seeded record cloud for the fixture: (xyz float64 (M,3), rgb float64 (M,3), colour level (M,3) uint8).  Colours are
    level / 255 like a camera's, so the reference's jittered colours are a function of (channel, level) and the fixture can
    hold them as a 3 x 256 table."""
    rng = np.random.RandomState(seed)
    xyz = rng.uniform(-0.5, 0.5, size=(num_points, 3)) * np.array([0.6, 0.4, 0.3]) + np.array([0.0, 0.4, 0.8])
    level = rng.randint(0, 256, size=(num_points, 3)).astype(np.uint8)
    return xyz, level.astype(np.float64) / 255.0, level


FIXTURE_CASES = (("m30000", 101, 30000, 2001), ("m9000", 102, 9000, 2002))      # name, cloud seed, points, np.random seed


def camera_frame(seed, num_points, T, bounds=DEFAULT_BOUNDS, nan_fraction=0.3, inside_fraction=0.5, margin=1e-9):
    """A seeded camera frame (float64 xyz (M,3) in CAMERA coordinates, rgb (M,3)): points spread over a box larger than the
    workspace, ``inside_fraction`` of them inside it, ``nan_fraction`` of the rows NaN (a depth camera's holes).  No
    transformed coordinate lies within ``margin`` of a bound: offenders are redrawn, so a difference in how the products
    are contracted cannot flip a predicate."""
    rng = np.random.RandomState(seed)
    x_hi, x_lo, z_hi, y_hi, y_lo = bounds
    lo_in, hi_in = np.array([x_lo, y_lo, z_hi - 0.5]), np.array([x_hi, y_hi, z_hi])
    Tinv = np.linalg.inv(np.asarray(T, dtype=np.float64))

    def draw(n):
        inside = rng.rand(n) < inside_fraction
        table = np.where(inside[:, None], rng.uniform(lo_in, hi_in, size=(n, 3)),
                         rng.uniform(lo_in - 0.6, hi_in + 0.6, size=(n, 3)))
        return table @ Tinv[:3, :3].T + Tinv[:3, 3]

    xyz = draw(num_points)
    for _ in range(100):
        t = transform_points(xyz, T)
        near = np.zeros(len(xyz), dtype=bool)
        for col, bound in ((0, x_hi), (0, x_lo), (2, z_hi), (1, y_hi), (1, y_lo)):
            near |= np.abs(t[:, col] - bound) < margin
        if not near.any():
            break
        xyz[near] = draw(int(near.sum()))
    else:
        raise AssertionError("camera_frame: could not clear the bounds' margins")
    rgb = rng.randint(0, 256, size=(num_points, 3)).astype(np.float64) / 255.0
    if nan_fraction:
        xyz[rng.rand(num_points) < nan_fraction] = np.nan
    return xyz, rgb
