// hand_field.h -- the body that retreat.hip's fan and hand_path.hip's paths share: the rigid hand at its final pose taken through
// K + 1 steps and read against the distance field at every one.  The two kernels differ in one thing, how step k takes a sample
// of the hand's local frame to a point of the volume's, and hand it in as to_volume(k, x, y, z, wx, wy, wz).
//
// One workgroup of HL_T threads per (grasp, candidate).  The lattice is the margin kernel's with standoff 0 and the walk is
// hand_lattice.h's: a thread decides a sample's membership once and then runs the K + 1 steps of that sample.  The per-step minima
// live in LDS, one word per step, not in registers: a thread compares its value with the word (a broadcast read) and issues the
// LDS integer min only when it would lower it -- the word only ever falls, so a stale read costs an atomic and never a result,
// and a minimum has no order.  The OUTSIDE count is one register per thread, summed by the wave butterfly and the four waves
// through LDS.  After one barrier threads 0..K store the profile and thread 0 walks the prefix.  Integer work only past the
// lookup: two runs give the same bytes.
#pragma once
#include "hand_lattice.h"

constexpr int HF_MAX_R = 16;         // candidates per grasp and steps per candidate: the entry points' documented limits
constexpr int HF_MAX_K = 64;

// pair: the workgroup's (grasp, candidate), its row of profile (K + 1 words, or null) and of result (4 words).  Every thread of
// the workgroup calls it; what the caller wrote to LDS before is visible after it (its first barrier follows the caller's stores).
template <bool SIGNED, typename ToVolume>
__device__ __forceinline__ void hand_steps(const int32_t* __restrict__ field, const VoxelGrid& grid, int outside,
                                           const GraspBox& box, float x_hi, const Lattice& lat, int K, int thresh, int64_t pair,
                                           int32_t* __restrict__ profile, int32_t* __restrict__ result, ToVolume to_volume) {
  __shared__ int step_min[HF_MAX_K + 1];
  __shared__ int red_out[HL_W];
  const int t = threadIdx.x;                         // (K + 1 <= 65 < HL_T: one step per thread)
  for (int k = t; k <= K; k += HL_T) step_min[k] = REGNET_EDT_NONE;
  int n_out = 0;
  __syncthreads();
  lattice_walk(lat, box, x_hi, [&](float x, float y, float z, const HandSets& in) {
    if (!(in.back || in.finger)) return;             // only the hand at its final pose moves; membership is decided once
    for (int k = 0; k <= K; ++k) {
      float wx, wy, wz;
      to_volume(k, x, y, z, wx, wy, wz);
      int value;
      const FieldLookup at = field_lookup<SIGNED>(field, grid, outside, wx, wy, wz, value);
      if (!at.inside) {
        n_out += (int)(k > 0);
        if (!at.has_value) continue;                 // an OUTSIDE sample under outside = 0: counted and skipped
      }
      if (value < step_min[k]) atomicMin(&step_min[k], value);
    }
  });
  n_out = wave_sum(n_out);
  block_put(n_out, red_out);
  __syncthreads();
  if (profile && t <= K) profile[pair * (K + 1) + t] = step_min[t];
  if (t == 0) {
    int free_steps = 0, free_min = REGNET_EDT_NONE, all_min = REGNET_EDT_NONE;
    bool open = true;
    for (int k = 1; k <= K; ++k) {
      const int m = step_min[k];
      all_min = min(all_min, m);
      open = open && m >= thresh;
      if (open) {
        free_steps = k;
        free_min = min(free_min, m);
      }
    }
    int32_t* out = result + pair * 4;
    out[0] = free_steps;
    out[1] = free_min;
    out[2] = all_min;
    out[3] = block_sum<HL_W>(red_out);
  }
}
