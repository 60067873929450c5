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

// Canonical dot product, under the same rule: ((ax*bx)+(ay*by))+(az*bz).
__device__ __forceinline__ float dot3(float ax, float ay, float az, float bx, float by, float bz) {
  float xx = ax * bx, yy = ay * by, zz = az * bz;
  float s = xx + yy;
  return s + zz;
}

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
