// tsdf_volume.h -- the layout of a TSDF volume of n = nx * ny * nz voxels (tsdf.hip writes it, approach_volume.hip and tsdf_mesh.hip
// read it), and the predicate of the surface extraction, which tsdf.hip's two passes and tsdf_mesh.hip's row lookup share:
// five planes of n 32-bit words in one allocation, the distance D at 0, the weight W at n, the colours after; voxel (ix, iy, iz)
// at word (iz * ny + iy) * nx + ix of each, its centre at o + (i + 0.5) * voxel along every axis.
#pragma once
#include "common.h"

struct Planes {
  float* D;
  int32_t* W;
  float* C[3];
};

__host__ __device__ __forceinline__ Planes planes_of(void* volume, long long n) {
  Planes p;
  p.D = (float*)volume;
  p.W = (int32_t*)volume + n;
  p.C[0] = (float*)volume + 2 * n; p.C[1] = (float*)volume + 3 * n; p.C[2] = (float*)volume + 4 * n;
  return p;
}

template <typename I>   // the index type: int where n < 2^31 is known to the caller
__host__ __device__ __forceinline__ I voxel_index(int ix, int iy, int iz, int nx, int ny) { return ((I)iz * ny + iy) * nx + ix; }

__device__ __forceinline__ float centre(float o, int i, float voxel) { return o + (((float)i + 0.5f) * voxel); }

// ---- the surface extraction's candidates (include/regnet_hip.h "Extraction") ------------------------------------------------
struct ExtractArgs {
  int nx, ny, nz, n, min_weight;
};

// whether the candidate (l, axis) is kept, for the three axes: bit a of the result
__device__ __forceinline__ int tsdf_kept(const float* __restrict__ D, const int32_t* __restrict__ W, const ExtractArgs& a, int l,
                                         int ix, int iy, int iz, bool& observed) {
  const int w = W[l];
  observed = w >= a.min_weight;
  if (!observed) return 0;
  const float d = D[l];
  if (!(d < 1.0f)) return 0;
  const int inside[3] = {ix + 1 < a.nx, iy + 1 < a.ny, iz + 1 < a.nz};
  const int step[3] = {1, a.nx, a.nx * a.ny};
  int bits = 0;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    if (!inside[k]) continue;
    const int m = l + step[k];
    if (W[m] < a.min_weight) continue;
    const float dn = D[m];
    if (dn < 1.0f && ((d < 0.0f) != (dn < 0.0f))) bits |= 1 << k;
  }
  return bits;
}

__device__ __forceinline__ void tsdf_index(const ExtractArgs& a, int l, int& ix, int& iy, int& iz) {
  ix = l % a.nx;
  const int r = l / a.nx;
  iy = r % a.ny;
  iz = r / a.ny;
}
