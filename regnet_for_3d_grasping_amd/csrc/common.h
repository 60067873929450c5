// Shared helpers for libregnet_hip.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/regnet_hip.h"

#define REGNET_LAUNCH_CHECK()                      \
  do {                                             \
    hipError_t e__ = hipGetLastError();            \
    if (e__ != hipSuccess) return (int)e__;        \
  } while (0)

static inline hipStream_t as_stream(void* s) { return reinterpret_cast<hipStream_t>(s); }

// Canonical squared distance: three individually rounded products summed left to right,
// ((dx*dx)+(dy*dy))+(dz*dz).  The translation unit using it MUST be built with
// -ffp-contract=off (see csrc/build.py); the oracle (oracle/pn2_oracle.c) does the same.
__device__ __forceinline__ float sqdist3(float ax, float ay, float az, float bx, float by, float bz) {
  float dx = ax - bx, dy = ay - by, dz = az - bz;
  float xx = dx * dx, yy = dy * dy, zz = dz * dz;
  float s = xx + yy;
  return s + zz;
}

// Canonical dot product, under the same rule: ((ax*bx)+(ay*by))+(az*bz).  With a matrix row for a it is the rotation-only
// form of affine3 (normals, directions).
template <typename S>
__host__ __device__ __forceinline__ S dot3(S ax, S ay, S az, S bx, S by, S bz) {
  S xx = ax * bx, yy = ay * by, zz = az * bz;
  S s = xx + yy;
  return s + zz;
}

// Canonical affine row, one row of a rigid transform applied to a point: ((r0*x + r1*y) + r2*z) + r3, four individually rounded
// operations in that order.  -ffp-contract=off is mandatory here as for sqdist3: the numpy restatements under tests/ and
// oracle/collision_oracle.py round every product and sum on its own, and the kernels are compared with them bit for bit.
template <typename S>
__host__ __device__ __forceinline__ S affine3(S r0, S r1, S r2, S r3, S x, S y, S z) {
  return dot3(r0, r1, r2, x, y, z) + r3;
}
// ... with the row read from four consecutive words
template <typename S>
__host__ __device__ __forceinline__ S affine3(const S* r, S x, S y, S z) { return affine3(r[0], r[1], r[2], r[3], x, y, z); }

// The larger of a and b, NaN when either is one (IEEE 754-2019 maximum; fmaxf returns the OTHER operand, so a ReLU written
// with it turns a NaN activation into 0), +0 for (-0, +0); any other pair gives fmaxf's bits.  One v_maximum3_f32 on gfx950.
__device__ __forceinline__ float max_nan(float a, float b) { return __builtin_elementwise_maximum(a, b); }

__device__ __forceinline__ int lane_id() { return (int)(threadIdx.x & 63); }

// number of set bits of `mask` below this lane
__device__ __forceinline__ int mbcnt64(uint64_t mask) {
  return (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
}

// Wave-aggregated append: the lanes whose `flag` is set take consecutive slots behind `*counter`, in lane order, with one
// atomicAdd per wave -> this lane's slot, -1 without the flag.  Every lane of the wave must make the call.
__device__ __forceinline__ int wave_append(bool flag, int* counter) {
  const uint64_t votes = __ballot(flag);
  if (votes == 0ull) return -1;
  const int leader = __builtin_ctzll(votes);
  int base = 0;
  if (lane_id() == leader) base = atomicAdd(counter, (int)__popcll(votes));
  base = __shfl(base, leader, 64);
  return flag ? base + mbcnt64(votes) : -1;
}

// Wave reductions, the xor butterfly 32 -> 1: every lane ends with the result.
__device__ __forceinline__ int wave_sum(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}
__device__ __forceinline__ float wave_min(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fminf(v, __shfl_xor(v, o));
  return v;
}
__device__ __forceinline__ int wave_min(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o));
  return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
  return v;
}

// Workgroup reduction over WAVES waves, in two halves around ONE __syncthreads() of the caller's, so that everything a kernel
// reduces at a point shares that barrier and one lane-0 branch: after the wave reductions, block_put (every thread) leaves the
// wave's value in slot[WAVES] of LDS; after the barrier block_sum / block_min / block_max join the WAVES words -- called by every
// thread when every thread needs the result, or only by the thread that stores it.  Only for reductions whose result does not
// depend on the order: integer sums and float min / max.
template <typename T>
__device__ __forceinline__ void block_put(T wave_value, T* slot) {
  if (lane_id() == 0) slot[threadIdx.x >> 6] = wave_value;
}
template <int WAVES, typename T, typename Join>
__device__ __forceinline__ T block_join(const T* slot, Join join) {
  T v = slot[0];
#pragma unroll
  for (int w = 1; w < WAVES; ++w) v = join(v, slot[w]);
  return v;
}
template <int WAVES>
__device__ __forceinline__ int block_sum(const int* slot) { return block_join<WAVES>(slot, [](int a, int b) { return a + b; }); }
template <int WAVES>
__device__ __forceinline__ float block_min(const float* slot) { return block_join<WAVES>(slot, fminf); }
template <int WAVES>
__device__ __forceinline__ int block_min(const int* slot) { return block_join<WAVES>(slot, [](int a, int b) { return a < b ? a : b; }); }
template <int WAVES>
__device__ __forceinline__ float block_max(const float* slot) { return block_join<WAVES>(slot, fmaxf); }
