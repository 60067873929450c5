// hand_box.h -- the gripper model of the grasp kernels (region.hip: collision scan and antipodal statistics, approach.hip,
// approach_volume.hip): the box constants, a grasp's matrix rows in registers, and THE definition of the hand's sets, which
// include/regnet_hip.h documents.  The translation unit must be built with -ffp-contract=off (common.h: affine3).
#pragma once
#include "common.h"

struct GraspBox {   // the reference's box constants as float32 (what torch compares a float32 tensor against)
  float x_lo, x_hi, half_thickness, half_width, half_space, back_x;
};

struct GraspRows {  // rows 0..2 of one grasp's row-major matrix
  float r[3][4];
};

// the rows of matrix `grasp` of M, `stride` floats from one matrix to the next (16: whole 4x4s, 12: the three rows alone)
__device__ __forceinline__ GraspRows grasp_rows(const float* __restrict__ M, int64_t grasp, int stride) {
  const float* m = M + grasp * stride;
  GraspRows g;
#pragma unroll
  for (int k = 0; k < 12; ++k) g.r[k >> 2][k & 3] = m[k];
  return g;
}

__device__ __forceinline__ void grasp_apply(const GraspRows& g, float px, float py, float pz, float& x, float& y, float& z) {
  x = affine3(g.r[0], px, py, pz);
  y = affine3(g.r[1], px, py, pz);
  z = affine3(g.r[2], px, py, pz);
}

// The sets a point (x, y, z) of the grasp's local frame belongs to, for the box, the grasp's own x_hi and the far end of the
// sweep, sweep_lo = x_lo - standoff.  Every comparison is strict: a point on a face is out, a NaN coordinate is in nothing.
struct HandSets {
  bool section;   // inside the hand's cross-section
  bool inner;     // ... and between the fingers' inner faces
  bool close;     // x in the closing slab, whatever y and z
  bool region;    // between the fingers: the closing region
  bool back;      // behind the palm
  bool finger;    // inside either finger
  bool blocker;   // in the way of the hand swept back along -approach
  float retreat;  // how far the hand has to retreat to clear the point
};

__device__ __forceinline__ HandSets hand_sets(const GraspBox& box, float x_hi, float sweep_lo, float x, float y, float z) {
  HandSets s;
  s.section = z < box.half_thickness && z > -box.half_thickness && y < box.half_width && y > -box.half_width;
  s.inner = s.section && y < box.half_space && y > -box.half_space;
  s.close = x > box.x_lo && x < x_hi;
  s.region = s.inner && s.close;
  s.back = s.section && s.close && x < box.back_x;
  const bool left = y > box.half_space, right = y < -box.half_space;
  s.finger = s.section && s.close && (left || right);
  const float front = s.inner ? box.back_x : x_hi;
  s.blocker = s.section && x < front && x > sweep_lo;
  s.retreat = fmaxf(box.x_lo - x, 0.0f);
  return s;
}
