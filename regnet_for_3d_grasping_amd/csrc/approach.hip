// approach.hip -- per-grasp approach clearance, closing extent and contact check on the device (gfx950): the step between "a
// collision-free grasp" and "a motion".  The collision scan beside it (region.hip: grasp_collision_kernel) tests the hand at the
// final pose only; this one also sweeps the hand back along -approach, measures the object between the fingers and judges the
// two contact bands on the observed cloud's normals.
//
// One workgroup per grasp, the cloud walked twice in the grasp's local frame, with region.hip's arithmetic restated (this file
// does not include it): x = ((t00*px + t01*py) + t02*pz) + t03 and likewise y, z, individually rounded fp32 in the written order
// (built with -ffp-contract=off), every comparison strict.  A point with a NaN coordinate has NaN local coordinates and is in
// nothing.  With ht / hw / hs the half thickness / half width / half space, xh the grasp's x_hi and S the standoff:
//   section = |z| < ht && |y| < hw          inner = section && |y| < hs          region = inner && x_lo < x < xh
//   pass 1: n_region, y_min / y_max / x_min over the region; n_hand = (behind the hand) + (inside a finger) as region.hip counts
//           them; the blockers of the sweep, section && x < front && x > x_lo - S with front = back_x for inner points and xh in
//           the finger lanes, their number and the least retreat s = fmaxf(x_lo - x, 0): clearance = fminf(S, min s).
//   pass 2 (normals given and the region not empty): band = min((y_max - y_min) / 3, contact_depth); per band (y > y_max - band,
//           y < y_min + band, grasp_antipodal_kernel's rule) its size and how many of its points have
//           |(t10*nx + t11*ny) + t12*nz| >= cos_friction.
// Only integer sums and float min / max are reduced (wave butterfly, then the four waves through LDS): no floating-point sum and
// no atomic, so the result does not depend on the order of anything.  Plain vector stores by thread 0.
#include "common.h"

namespace {

constexpr int AP_T = 256;
constexpr int AP_W = AP_T / 64;

struct GraspBox {   // the reference's box constants as float32, as in region.hip
  float x_lo, x_hi, half_thickness, half_width, half_space, back_x;
};

// local coordinates of point j for the matrix rows held in registers: region.hip's GC_LOCAL, restated
#define AP_LOCAL(j)                                                          \
  const float* p = points + (int64_t)(j) * pn;                               \
  const float px = p[0], py = p[pc], pz = p[2 * pc];                         \
  const float x = ((t00 * px + t01 * py) + t02 * pz) + t03;                  \
  const float y = ((t10 * px + t11 * py) + t12 * pz) + t13;                  \
  const float z = ((t20 * px + t21 * py) + t22 * pz) + t23;                  \
  const bool section = z < box.half_thickness && z > -box.half_thickness && y < box.half_width && y > -box.half_width; \
  const bool inner = section && y < box.half_space && y > -box.half_space;   \
  const bool close = x > box.x_lo && x < x_hi;                               \
  const bool region = inner && close;

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
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
  return v;
}

__global__ __launch_bounds__(AP_T) void approach_kernel(const float* __restrict__ points, int64_t pn, int64_t pc,
                                                        const float* __restrict__ normals, int64_t nn, int64_t nc, int N,
                                                        const float* __restrict__ T, GraspBox box,
                                                        const float* __restrict__ x_hi_per_grasp, float standoff,
                                                        float contact_depth, float cos_friction,
                                                        int32_t* __restrict__ counts, float* __restrict__ values) {
  __shared__ int red_i[4][AP_W];
  __shared__ float red_f[4][AP_W];
  const float* t = T + (int64_t)blockIdx.x * 16;
  const float t00 = t[0], t01 = t[1], t02 = t[2], t03 = t[3];
  const float t10 = t[4], t11 = t[5], t12 = t[6], t13 = t[7];
  const float t20 = t[8], t21 = t[9], t22 = t[10], t23 = t[11];
  const float x_hi = x_hi_per_grasp ? x_hi_per_grasp[blockIdx.x] : box.x_hi;
  const float sweep_lo = box.x_lo - standoff;
  const int wave = threadIdx.x >> 6;
  const bool lead = (threadIdx.x & 63) == 0;

  int n_region = 0, n_block = 0, n_hand = 0;
  float y_min = __builtin_inff(), y_max = -__builtin_inff(), x_min = __builtin_inff(), s_min = __builtin_inff();
  for (int64_t j = threadIdx.x; j < N; j += AP_T) {   // (64-bit: j + AP_T may pass 2^31)
    AP_LOCAL(j)
    if (region) {
      n_region += 1;
      y_min = fminf(y_min, y);
      y_max = fmaxf(y_max, y);
      x_min = fminf(x_min, x);
    }
    const bool back = section && close && x < box.back_x;
    const bool finger = section && close && (y > box.half_space || y < -box.half_space);
    n_hand += (int)back + (int)finger;
    const float front = inner ? box.back_x : x_hi;
    if (section && x < front && x > sweep_lo) {
      n_block += 1;
      s_min = fminf(s_min, fmaxf(box.x_lo - x, 0.0f));
    }
  }
  n_region = wave_sum(n_region); n_block = wave_sum(n_block); n_hand = wave_sum(n_hand);
  y_min = wave_min(y_min); y_max = wave_max(y_max); x_min = wave_min(x_min); s_min = wave_min(s_min);
  if (lead) {
    red_i[0][wave] = n_region; red_i[1][wave] = n_block; red_i[2][wave] = n_hand;
    red_f[0][wave] = y_min; red_f[1][wave] = y_max; red_f[2][wave] = x_min; red_f[3][wave] = s_min;
  }
  __syncthreads();
  n_region = n_block = n_hand = 0;
#pragma unroll
  for (int w = 0; w < AP_W; ++w) {
    n_region += red_i[0][w]; n_block += red_i[1][w]; n_hand += red_i[2][w];
    y_min = fminf(y_min, red_f[0][w]); y_max = fmaxf(y_max, red_f[1][w]);
    x_min = fminf(x_min, red_f[2][w]); s_min = fminf(s_min, red_f[3][w]);
  }

  int n_left = 0, ok_left = 0, n_right = 0, ok_right = 0;
  if (normals != nullptr && n_region > 0) {      // (uniform over the workgroup: every thread holds the reduced values)
    const float third = (y_max - y_min) / 3.0f;
    const float band = third < contact_depth ? third : contact_depth;
    const float left_edge = y_max - band, right_edge = y_min + band;
    for (int64_t j = threadIdx.x; j < N; j += AP_T) {
      AP_LOCAL(j)
      if (!region) continue;
      const bool left = y > left_edge, right = y < right_edge;
      if (!(left || right)) continue;
      const float* q = normals + j * nn;
      const bool ok = fabsf((t10 * q[0] + t11 * q[nc]) + t12 * q[2 * nc]) >= cos_friction;   // (a NaN normal fails)
      n_left += (int)left; ok_left += (int)(left && ok);
      n_right += (int)right; ok_right += (int)(right && ok);
    }
    n_left = wave_sum(n_left); ok_left = wave_sum(ok_left); n_right = wave_sum(n_right); ok_right = wave_sum(ok_right);
    __syncthreads();                              // pass 1's reads of red_i are done
    if (lead) { red_i[0][wave] = n_left; red_i[1][wave] = ok_left; red_i[2][wave] = n_right; red_i[3][wave] = ok_right; }
    __syncthreads();
    n_left = ok_left = n_right = ok_right = 0;
#pragma unroll
    for (int w = 0; w < AP_W; ++w) {
      n_left += red_i[0][w]; ok_left += red_i[1][w]; n_right += red_i[2][w]; ok_right += red_i[3][w];
    }
  }
  if (threadIdx.x == 0) {
    int32_t* c = counts + (int64_t)blockIdx.x * 8;
    c[0] = n_region; c[1] = n_block; c[2] = n_hand; c[3] = n_left; c[4] = ok_left; c[5] = n_right; c[6] = ok_right; c[7] = 0;
    float* v = values + (int64_t)blockIdx.x * 4;
    v[0] = y_min + 0.0f; v[1] = y_max + 0.0f; v[2] = fminf(standoff, s_min) + 0.0f; v[3] = x_min + 0.0f;   // (+ 0.0f: no -0.0)
  }
}

}  // namespace

extern "C" int regnet_grasp_approach_f32(const float* points, int64_t pn, int64_t pc, const float* normals, int64_t nn,
                                         int64_t nc, int64_t N, const float* T, int64_t B, float x_lo, float x_hi,
                                         const float* x_hi_per_grasp, float half_thickness, float half_width, float half_space,
                                         float back_x, float standoff, float contact_depth, float cos_friction, int32_t* counts,
                                         float* values, void* stream) {
  if (N < 0 || B < 0) return REGNET_ERR_SHAPE;
  if (N >= (int64_t)1 << 31 || B >= (int64_t)1 << 31) return REGNET_ERR_UNSUPPORTED;
  if (!(standoff >= 0.0f) || standoff == __builtin_inff()) return REGNET_ERR_UNSUPPORTED;   // negative, NaN or infinite
  if (B == 0) return REGNET_OK;
  if (!T || !counts || !values || (N > 0 && !points)) return REGNET_ERR_NULL;
  const GraspBox box{x_lo, x_hi, half_thickness, half_width, half_space, back_x};
  hipLaunchKernelGGL(approach_kernel, dim3((unsigned)B), dim3(AP_T), 0, as_stream(stream), points, pn, pc, normals, nn, nc,
                     (int)N, T, box, x_hi_per_grasp, standoff, contact_depth, cos_friction, counts, values);
  REGNET_LAUNCH_CHECK();
  return REGNET_OK;
}
