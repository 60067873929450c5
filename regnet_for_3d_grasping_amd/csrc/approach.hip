// approach.hip -- per-grasp approach clearance, closing extent and contact check on the device (gfx950): the step between "a
// collision-free grasp" and "a motion".  The collision scan beside it (region.hip: grasp_collision_kernel) tests the hand at the
// final pose only; this one also sweeps the hand back along -approach, measures the object between the fingers and judges the
// two contact bands on the observed cloud's normals.
//
// One workgroup per grasp, the cloud walked twice in the grasp's local frame.  The local coordinates and the sets of a point
// (section, inner, region, back, finger, blocker, retreat) are hand_box.h's, the one definition this kernel shares with
// region.hip's collision scan and with approach_volume.hip: individually rounded fp32 in the written order (built with
// -ffp-contract=off), every comparison strict, a NaN coordinate in nothing.  With xh the grasp's x_hi and S the standoff:
//   pass 1: n_region, y_min / y_max / x_min over the region; n_hand = back + finger; the blockers of the sweep, their number and
//           their least retreat: clearance = fminf(S, min retreat).
//   pass 2 (normals given and the region not empty): band = min((y_max - y_min) / 3, contact_depth); per band (y > y_max - band,
//           y < y_min + band, grasp_antipodal_kernel's rule) its size and how many of its points have
//           |(t10*nx + t11*ny) + t12*nz| >= cos_friction.
// Only integer sums and float min / max are reduced (common.h: the wave butterfly, then the waves through LDS): no floating-point sum and no atomic, so
// the result does not depend on the order of anything.  Plain vector stores by thread 0.
#include "hand_box.h"

namespace {

constexpr int AP_T = 256;
constexpr int AP_W = AP_T / 64;

__global__ __launch_bounds__(AP_T) void approach_kernel(const float* __restrict__ points, int64_t pn, int64_t pc,
                                                        const float* __restrict__ normals, int64_t nn, int64_t nc, int N,
                                                        const float* __restrict__ T, GraspBox box,
                                                        const float* __restrict__ x_hi_per_grasp, float standoff,
                                                        float contact_depth, float cos_friction,
                                                        int32_t* __restrict__ counts, float* __restrict__ values) {
  __shared__ int red_i[4][AP_W];
  __shared__ float red_f[4][AP_W];
  const GraspRows g = grasp_rows(T, blockIdx.x, 16);
  const float x_hi = x_hi_per_grasp ? x_hi_per_grasp[blockIdx.x] : box.x_hi;
  const float sweep_lo = box.x_lo - standoff;

  int n_region = 0, n_block = 0, n_hand = 0;
  float y_min = __builtin_inff(), y_max = -__builtin_inff(), x_min = __builtin_inff(), s_min = __builtin_inff();
  for (int64_t j = threadIdx.x; j < N; j += AP_T) {   // (64-bit: j + AP_T may pass 2^31)
    const float* p = points + j * pn;
    float x, y, z;
    grasp_apply(g, p[0], p[pc], p[2 * pc], x, y, z);
    const HandSets s = hand_sets(box, x_hi, sweep_lo, x, y, z);
    if (s.region) {
      n_region += 1;
      y_min = fminf(y_min, y);
      y_max = fmaxf(y_max, y);
      x_min = fminf(x_min, x);
    }
    n_hand += (int)s.back + (int)s.finger;
    if (s.blocker) {
      n_block += 1;
      s_min = fminf(s_min, s.retreat);
    }
  }
  n_region = wave_sum(n_region); n_block = wave_sum(n_block); n_hand = wave_sum(n_hand);
  y_min = wave_min(y_min); y_max = wave_max(y_max); x_min = wave_min(x_min); s_min = wave_min(s_min);
  block_put(n_region, red_i[0]); block_put(n_block, red_i[1]); block_put(n_hand, red_i[2]);
  block_put(y_min, red_f[0]); block_put(y_max, red_f[1]); block_put(x_min, red_f[2]); block_put(s_min, red_f[3]);
  __syncthreads();
  n_region = block_sum<AP_W>(red_i[0]); n_block = block_sum<AP_W>(red_i[1]);
  n_hand = block_sum<AP_W>(red_i[2]);
  y_min = block_min<AP_W>(red_f[0]); y_max = block_max<AP_W>(red_f[1]);
  x_min = block_min<AP_W>(red_f[2]); s_min = block_min<AP_W>(red_f[3]);

  int n_left = 0, ok_left = 0, n_right = 0, ok_right = 0;
  if (normals != nullptr && n_region > 0) {      // (uniform over the workgroup: every thread holds the reduced values)
    const float third = (y_max - y_min) / 3.0f;
    const float band = third < contact_depth ? third : contact_depth;
    const float left_edge = y_max - band, right_edge = y_min + band;
    for (int64_t j = threadIdx.x; j < N; j += AP_T) {
      const float* p = points + j * pn;
      float x, y, z;
      grasp_apply(g, p[0], p[pc], p[2 * pc], x, y, z);
      if (!hand_sets(box, x_hi, sweep_lo, x, y, z).region) continue;
      const bool left = y > left_edge, right = y < right_edge;
      if (!(left || right)) continue;
      const float* q = normals + j * nn;
      const bool ok = fabsf(dot3(g.r[1][0], g.r[1][1], g.r[1][2], q[0], q[nc], q[2 * nc])) >= cos_friction;   // (a NaN normal fails)
      n_left += (int)left; ok_left += (int)(left && ok);
      n_right += (int)right; ok_right += (int)(right && ok);
    }
    n_left = wave_sum(n_left); ok_left = wave_sum(ok_left); n_right = wave_sum(n_right); ok_right = wave_sum(ok_right);
    __syncthreads();                              // pass 1's reads of red_i are done
    block_put(n_left, red_i[0]); block_put(ok_left, red_i[1]); block_put(n_right, red_i[2]); block_put(ok_right, red_i[3]);
    __syncthreads();
    n_left = block_sum<AP_W>(red_i[0]); ok_left = block_sum<AP_W>(red_i[1]);
    n_right = block_sum<AP_W>(red_i[2]); ok_right = block_sum<AP_W>(red_i[3]);
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
