// ray_clip.h -- the slab clip of a sampled camera ray against a voxel box, shared by tsdf.hip's raycast and view_gain.hip's march
// (include/regnet_hip.h, regnet_tsdf_raycast_f32 "clip").  It changes which samples a ray visits and no bit of a result: a sample it
// leaves out cannot lie inside the box, for the interpolated lookup (the box of voxel centres) or the nearest one (the box of voxels,
// half a voxel larger, which the margin of one voxel covers).
#pragma once
#include "common.h"

constexpr double RAY_CLIP_SLACK = 1.0 / 262144.0;   // 2^-18: 64 float32 roundings of the clip's magnitudes

// the samples [first, last] outside which the ray's point cannot lie inside the box of voxel centres: a slab test in float64 on
// the exact ray t + z d, the box grown by a voxel and by RAY_CLIP_SLACK of every magnitude that enters the float32 point (64 times
// the roundings of the ray point and the cell), the range grown by a sample either way.  A NaN constrains nothing.  r: rows 0..2 of
// the camera-to-common transform; (du, dv) = ((float)u - cx, (float)v - cy); first > last: no sample.
__device__ __forceinline__ void ray_clip(const float* r, const int* n, const float* o, float voxel, float near_f, float step_f,
                                         int n_steps, float du, float dv, float rfx, float rfy, int& first, int& last) {
  const double near = (double)near_f, step = (double)step_f;
  const double far = near + (double)(n_steps - 1) * step;
  const double dcx = (double)du * (double)rfx, dcy = (double)dv * (double)rfy;
  const double zs = RAY_CLIP_SLACK * (fabs(near) + far);
  double za = near - zs, zb = far + zs;
  bool empty = false;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const double r0 = (double)r[4 * k], r1 = (double)r[4 * k + 1], r2 = (double)r[4 * k + 2], t = (double)r[4 * k + 3];
    const double d = (r0 * dcx + r1 * dcy) + r2;
    const double ok = (double)o[k], vx = (double)voxel, extent = (double)n[k] * vx;
    const double reach = (fabs(r0 * dcx) + fabs(r1 * dcy) + fabs(r2)) * far;
    const double m = vx + RAY_CLIP_SLACK * (fabs(t) + reach + fabs(ok) + extent);
    const double lo = ok + 0.5 * vx - m, hi = ok + extent - 0.5 * vx + m;
    if (d == 0.0) {
      empty = empty || t < lo || t > hi;
    } else {
      const double z1 = (lo - t) / d, z2 = (hi - t) / d;
      za = fmax(za, fmin(z1, z2));
      zb = fmin(zb, fmax(z1, z2));
    }
  }
  if (empty || za > zb) { first = 1; last = 0; return; }
  const double top = (double)(n_steps - 1);
  first = (int)fmin(fmax(floor((za - near) / step) - 1.0, 0.0), top);
  last = (int)fmin(fmax(ceil((zb - near) / step) + 1.0, 0.0), top);
}
