"""numpy restatement of the TSDF volume (include/regnet_hip.h, DESIGN.md par. 5 "TSDF volume"), written from the contract text
and not from csrc/tsdf.hip: float32 arrays, one operation per statement (numpy rounds each on its own; its division and square
root are correctly rounded), a Python loop over the views, plain boolean masks.  The volume is held as ``D`` (N) float32, ``W`` (N)
int32 and ``C`` (N,3) float32 with voxel (ix, iy, iz) at ``(iz ny + iy) nx + ix``.
"""
import numpy as np

f32 = np.float32
UPDATED, NOT_IN_VIEW, NO_DEPTH, BEHIND = 0, 1, 2, 3
DEFAULTS = dict(voxel=0.002, trunc=0.01, origin=(-0.32, -0.32, 0.3), dims=(320, 320, 320), max_weight=255, min_weight=1,
                max_points=1 << 20)


def constants(voxel, trunc):
    """-> (voxel_f, trunc_f, rtrunc): evaluated in float64, rounded once."""
    return f32(float(voxel)), f32(float(trunc)), f32(1.0 / float(trunc))


def camera_from_common(pose):
    """The view's camera-to-common pose (None: identity) -> 12 float32 of its float64 inverse."""
    T = np.eye(4) if pose is None else np.asarray(pose, dtype=np.float64)
    return np.linalg.inv(T)[:3, :].reshape(12).astype(np.float32)


class Volume:
    def __init__(self, **params):
        p = dict(DEFAULTS)
        p.update(params)
        self.p = p
        self.dims = tuple(int(d) for d in p["dims"])
        self.n = self.dims[0] * self.dims[1] * self.dims[2]
        self.origin = np.asarray(p["origin"], dtype=np.float64).astype(np.float32)
        self.voxel, self.trunc, self.rtrunc = constants(p["voxel"], p["trunc"])
        self.reset()

    def reset(self):
        self.D = np.ones((self.n,), dtype=np.float32)
        self.W = np.zeros((self.n,), dtype=np.int32)
        self.C = np.zeros((self.n, 3), dtype=np.float32)

    def indices(self):
        """-> (ix, iy, iz) of every linear index, int64."""
        nx, ny, _ = self.dims
        l = np.arange(self.n, dtype=np.int64)
        return l % nx, (l // nx) % ny, l // (nx * ny)

    def centres(self):
        """p_k = o_k + ((float)i_k + 0.5f) * voxel -> (N,3) float32."""
        out = []
        for k, i in enumerate(self.indices()):
            a = i.astype(np.float32) + f32(0.5)
            b = a * self.voxel
            out.append(self.origin[k] + b)
        p = np.stack(out, axis=1)
        assert p.dtype == np.float32
        return p

    def integrate(self, xyz, rgb, width, height, intrinsics, pose=None):
        """One view -> counts (4) int32 = (updated, not in view, no depth, behind)."""
        W, H = int(width), int(height)
        xyz = np.asarray(xyz, dtype=np.float32).reshape(H * W, 3)
        rgb = np.zeros((H * W, 3), dtype=np.float32) if rgb is None else np.asarray(rgb, dtype=np.float32).reshape(H * W, 3)
        fx, fy, cx, cy = (f32(float(v)) for v in intrinsics)
        r = camera_from_common(pose)
        p = self.centres()
        px, py, pz = p[:, 0], p[:, 1], p[:, 2]
        with np.errstate(all="ignore"):
            cam = []
            for k in range(3):
                a = r[4 * k] * px
                b = r[4 * k + 1] * py
                c = r[4 * k + 2] * pz
                s = a + b
                s = s + c
                cam.append(s + r[4 * k + 3])
            x, y, z = cam
            front = np.isfinite(z) & (z > 0)
            qx = x / z
            qy = y / z
            u = qx * fx
            u = u + cx
            v = qy * fy
            v = v + cy
            fu = np.floor(u + f32(0.5))
            fv = np.floor(v + f32(0.5))
            assert fu.dtype == fv.dtype == np.float32
            in_view = front & (fu >= 0) & (fu < f32(W)) & (fv >= 0) & (fv < f32(H))
            pixel = np.where(in_view, fv, 0).astype(np.int64) * W + np.where(in_view, fu, 0).astype(np.int64)
            zd = xyz[pixel, 2]
            has_depth = in_view & np.isfinite(zd)
            sdf = zd - z
            behind = has_depth & (sdf < -self.trunc)
            update = has_depth & ~behind
            t = np.minimum(sdf * self.rtrunc, f32(1.0))
            wf = self.W.astype(np.float32)
            w1 = wf + f32(1.0)
            d = self.D * wf
            d = d + t
            d = d / w1
            colour = rgb[pixel]
            c = self.C * wf[:, None]
            c = c + colour
            c = c / w1[:, None]
        assert d.dtype == c.dtype == t.dtype == np.float32
        self.D = np.where(update, d, self.D)
        self.C = np.where(update[:, None], c, self.C)
        self.W = np.where(update, np.minimum(self.W + 1, np.int32(min(int(self.p["max_weight"]), 2 ** 31 - 1))), self.W).astype(np.int32)
        return np.array([update.sum(), (~in_view).sum(), (in_view & ~has_depth).sum(), behind.sum()], dtype=np.int32)

    def _shift(self, a, axis, by, fill):
        """``a`` (N,...) read at voxel + by * e_axis; ``fill`` where that voxel is outside -> (values, inside)."""
        nx, ny, nz = self.dims
        i = self.indices()[axis] + by
        inside = (i >= 0) & (i < self.dims[axis])
        step = (1, nx, nx * ny)[axis] * by
        l = np.where(inside, np.arange(self.n, dtype=np.int64) + step, 0)
        vals = a[l]
        mask = inside if vals.ndim == 1 else inside[:, None]
        return np.where(mask, vals, fill), inside

    def gradient(self):
        """Per voxel and axis the central, or doubled one-sided, difference of D over the usable neighbours -> (N,3) float32."""
        mw = np.int32(self.p["min_weight"])
        out = []
        with np.errstate(all="ignore"):
            for k in range(3):
                d_lo, in_lo = self._shift(self.D, k, -1, f32(0))
                d_hi, in_hi = self._shift(self.D, k, +1, f32(0))
                w_lo, _ = self._shift(self.W, k, -1, np.int32(0))
                w_hi, _ = self._shift(self.W, k, +1, np.int32(0))
                lo = in_lo & (w_lo >= mw)
                hi = in_hi & (w_hi >= mw)
                both = d_hi - d_lo
                only_hi = (d_hi - self.D) * f32(2.0)
                only_lo = (self.D - d_lo) * f32(2.0)
                g = np.where(lo & hi, both, np.where(hi, only_hi, np.where(lo, only_lo, f32(0))))
                assert g.dtype == np.float32
                out.append(g)
        return np.stack(out, axis=1)

    def extract(self):
        """-> dict(xyz, rgb, normal (max_points,3) float32, weight (max_points) int32, num (4) int32, keys (K) int64)."""
        mw = np.int32(self.p["min_weight"])
        mp = int(self.p["max_points"])
        p = self.centres()
        grad = self.gradient()
        rows = []
        with np.errstate(all="ignore"):
            for a in range(3):
                d_n, inside = self._shift(self.D, a, +1, f32(1))
                w_n, _ = self._shift(self.W, a, +1, np.int32(0))
                c_n, _ = self._shift(self.C, a, +1, f32(0))
                g_n, _ = self._shift(grad, a, +1, f32(0))
                keep = inside & (self.W >= mw) & (w_n >= mw) & (self.D < 1) & (d_n < 1) & ((self.D < 0) != (d_n < 0))
                den = self.D - d_n
                s = self.D / den
                xyz = p.copy()
                step = s * self.voxel
                xyz[:, a] = p[:, a] + step
                dc = c_n - self.C
                dc = s[:, None] * dc
                rgb = self.C + dc
                dg = g_n - grad
                dg = s[:, None] * dg
                g = grad + dg
                len2 = g[:, 0] * g[:, 0]
                len2 = len2 + g[:, 1] * g[:, 1]
                len2 = len2 + g[:, 2] * g[:, 2]
                ok = np.isfinite(len2) & (len2 > 0)
                normal = g / np.sqrt(len2)[:, None]
                normal = np.where(ok[:, None], normal, f32(np.nan))
                weight = np.minimum(self.W, w_n)
                assert xyz.dtype == rgb.dtype == normal.dtype == np.float32
                l = np.nonzero(keep)[0]
                rows.append((3 * l + a, xyz[l], rgb[l], normal[l], weight[l]))
        keys = np.concatenate([r[0] for r in rows])
        order = np.argsort(keys, kind="stable")
        total = len(keys)
        K = min(total, mp)
        order = order[:K]
        out = {"xyz": np.full((mp, 3), np.nan, dtype=np.float32), "rgb": np.zeros((mp, 3), dtype=np.float32),
               "normal": np.full((mp, 3), np.nan, dtype=np.float32), "weight": np.full((mp,), -1, dtype=np.int32)}
        for j, name in enumerate(("xyz", "rgb", "normal", "weight")):
            out[name][:K] = np.concatenate([r[j + 1] for r in rows])[order]
        out["keys"] = keys[order]
        out["num"] = np.array([K, total, (self.W >= mw).sum(), 1 if total > mp else 0], dtype=np.int32)
        return out


def fuse_volume(clouds, shapes, poses=None, **params):
    """``clouds``: per view ``(xyz, rgb)`` (rgb may be None); ``shapes``: per view ``(width, height, intrinsics)``; ``poses``: per
    view the camera-to-common 4x4 or None -> (Volume, counts (V,4) int32, the extraction's dict): reset, integrate in view order,
    extract."""
    vol = Volume(**params)
    poses = [None] * len(clouds) if poses is None else list(poses)
    counts = [vol.integrate(xyz, rgb, w, h, k, pose) for (xyz, rgb), (w, h, k), pose in zip(clouds, shapes, poses)]
    return vol, np.stack(counts), vol.extract()
