// sdf_sample.h -- the signed field read at a point (include/regnet_hip.h "signed metres", "signed query"): a signed word as
// metres, and the trilinear interpolant between the eight voxel centres around a point with its analytic gradient.  Shared by
// edt.hip's signed query (one lane per point) and hand_adjust.hip's push-out (every hand sample at every iterate), which must
// agree to the bit.  The translation unit must be built with -ffp-contract=off (hand_box.h).
#pragma once
#include "hand_lattice.h"

// a signed word s: a = sqrtf((float)|s|), then (a - 0.5f) * voxel with the sign of s -- the distance to the boundary FACE between
// the classes, not to a voxel centre; every operation rounded on its own
__device__ __forceinline__ float sdf_metres(int s, float voxel) {
  const int a2 = s < 0 ? -s : s;
  if (a2 >= REGNET_EDT_NONE) return s < 0 ? -__builtin_inff() : __builtin_inff();
  const float a = sqrtf((float)a2);
  const float h = a - 0.5f;
  const float m = h * voxel;
  return copysignf(m, (float)s) + 0.0f;
}

__device__ __forceinline__ float sdf_lerp(float a, float b, float t) {
  const float d = b - a;
  const float s = t * d;
  return a + s;
}

// one axis of the trilinear query: u = (w - o) / voxel - 0.5, the two corner indices clamped into the lattice, and the weight
__device__ __forceinline__ void sdf_axis(float w, float o, float voxel, int n, int& i0, int& i1, float& t) {
  const float u = __fdiv_rn(w - o, voxel) - 0.5f;
  const float f = floorf(u);
  t = u - f;
  const int i = (int)f;                              // (the point is INSIDE: -1 <= f <= n - 1)
  i0 = min(max(i, 0), n - 1);
  i1 = min(max(i + 1, 0), n - 1);
}

// The interpolated signed metres at the point (wx, wy, wz) of the grid's frame, which must be INSIDE (grid_voxel), and with
// `gradient` the derivative of the interpolant in the grid's frame; without it gx, gy and gz are left as they are.  Eight loads.
__device__ __forceinline__ float sdf_sample(const int32_t* __restrict__ field, const VoxelGrid& grid, float wx, float wy, float wz,
                                            bool gradient, float& gx, float& gy, float& gz) {
  const float vox = grid.voxel;
  int x0, x1, y0, y1, z0, z1;
  float tx, ty, tz;
  sdf_axis(wx, grid.ox, vox, grid.nx, x0, x1, tx);
  sdf_axis(wy, grid.oy, vox, grid.ny, y0, y1, ty);
  sdf_axis(wz, grid.oz, vox, grid.nz, z0, z1, tz);
  const int64_t r00 = ((int64_t)z0 * grid.ny + y0) * grid.nx, r10 = ((int64_t)z0 * grid.ny + y1) * grid.nx;
  const int64_t r01 = ((int64_t)z1 * grid.ny + y0) * grid.nx, r11 = ((int64_t)z1 * grid.ny + y1) * grid.nx;
  // c[z][y][x]
  const float c000 = sdf_metres(field[r00 + x0], vox), c001 = sdf_metres(field[r00 + x1], vox);
  const float c010 = sdf_metres(field[r10 + x0], vox), c011 = sdf_metres(field[r10 + x1], vox);
  const float c100 = sdf_metres(field[r01 + x0], vox), c101 = sdf_metres(field[r01 + x1], vox);
  const float c110 = sdf_metres(field[r11 + x0], vox), c111 = sdf_metres(field[r11 + x1], vox);
  if (gradient) {
    // per axis the four differences of the corner values along it over the voxel, lerped over the other two axes, x before y before z
    gx = sdf_lerp(sdf_lerp(__fdiv_rn(c001 - c000, vox), __fdiv_rn(c011 - c010, vox), ty),
                  sdf_lerp(__fdiv_rn(c101 - c100, vox), __fdiv_rn(c111 - c110, vox), ty), tz);
    gy = sdf_lerp(sdf_lerp(__fdiv_rn(c010 - c000, vox), __fdiv_rn(c011 - c001, vox), tx),
                  sdf_lerp(__fdiv_rn(c110 - c100, vox), __fdiv_rn(c111 - c101, vox), tx), tz);
    gz = sdf_lerp(sdf_lerp(__fdiv_rn(c100 - c000, vox), __fdiv_rn(c101 - c001, vox), tx),
                  sdf_lerp(__fdiv_rn(c110 - c010, vox), __fdiv_rn(c111 - c011, vox), tx), ty);
  }
  return sdf_lerp(sdf_lerp(sdf_lerp(c000, c001, tx), sdf_lerp(c010, c011, tx), ty),
                  sdf_lerp(sdf_lerp(c100, c101, tx), sdf_lerp(c110, c111, tx), ty), tz);
}
