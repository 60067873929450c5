// tsdf_volume.h -- the layout of a TSDF volume of n = nx * ny * nz voxels (tsdf.hip writes it, approach_volume.hip reads it):
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
