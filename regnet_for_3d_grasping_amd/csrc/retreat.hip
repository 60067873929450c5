// retreat.hip -- the retreat fan (include/regnet_hip.h "retreat fan"): the rigid hand at its final pose, moved along R candidate
// directions in K steps and read against the distance field at every step, and the pick of the best direction per grasp.
//
// One workgroup of HL_T threads per (grasp, direction), the body hand_field.h's hand_steps: step k translates the sample by
// k ds d in the grasp's local frame and then applies the grasp's own L.
#include "hand_field.h"

namespace {

struct Fan {
  int R, K;
  float ds;
  int thresh;
  int64_t dirs_grasp_stride;
};

template <bool SIGNED>
__global__ __launch_bounds__(HL_T) void retreat_fan_kernel(const int32_t* __restrict__ field, VoxelGrid grid, int outside,
                                                           const float* __restrict__ L, GraspBox box,
                                                           const float* __restrict__ x_hi_per_grasp, Lattice lat,
                                                           const float* __restrict__ dirs, Fan fan,
                                                           int32_t* __restrict__ profile, int32_t* __restrict__ result) {
  const int64_t pair = blockIdx.x;                   // (b, r), r fastest
  const int64_t b = pair / fan.R;
  const int r = (int)(pair - b * fan.R);
  const GraspRows g = grasp_rows(L, b, 12);
  const float x_hi = x_hi_per_grasp ? x_hi_per_grasp[b] : box.x_hi;
  const float* d = dirs + b * fan.dirs_grasp_stride + 3 * r;
  const float dx = d[0], dy = d[1], dz = d[2];
  const float ds = fan.ds;
  hand_steps<SIGNED>(field, grid, outside, box, x_hi, lat, fan.K, fan.thresh, pair, profile, result,
                     [&](int k, float x, float y, float z, float& wx, float& wy, float& wz) {
    const float t = (float)k * ds;
    const float px = x + (t * dx), py = y + (t * dy), pz = z + (t * dz);
    grasp_apply(g, px, py, pz, wx, wy, wz);
  });
}

// one lane per grasp: the direction with the most free steps, then the larger free-prefix minimum, then the smaller r
__global__ __launch_bounds__(HL_T) void retreat_pick_kernel(const int32_t* __restrict__ result, int64_t B, int R,
                                                            int32_t* __restrict__ best) {
  const int64_t b = (int64_t)blockIdx.x * HL_T + threadIdx.x;
  if (b >= B) return;
  const int32_t* row = result + b * R * 4;
  int pick = 0, steps = row[0], margin = row[1];
  for (int r = 1; r < R; ++r) {
    const int s = row[4 * r], m = row[4 * r + 1];
    if (s > steps || (s == steps && m > margin)) {
      pick = r; steps = s; margin = m;
    }
  }
  int32_t* out = best + b * 4;
  out[0] = pick; out[1] = steps; out[2] = margin; out[3] = 0;
}

template <bool SIGNED>
int retreat_fan(const int32_t* field, int64_t nx, int64_t ny, int64_t nz, const float* origin3, double voxel, int outside,
                const float* L, int64_t B, float x_lo, float x_hi, const float* x_hi_per_grasp, float half_thickness,
                float half_width, float half_space, float back_x, double step, float x_extent, const float* dirs,
                int64_t dirs_grasp_stride, int64_t R, int64_t K, double ds, int thresh, int32_t* profile, int32_t* result,
                void* stream) {
  if (R < 1 || K < 1 || dirs_grasp_stride < 0) return REGNET_ERR_SHAPE;   // (with the opening checks' own SHAPE rules: one status)
  LatticeCall call;
  int status = field_call_checks(nx, ny, nz, voxel, outside, B, step, &call);
  if (status != REGNET_OK) return status;
  if (R > HF_MAX_R || K > HF_MAX_K || B * R * (K + 1) > ((int64_t)1 << 28)) return REGNET_ERR_UNSUPPORTED;
  const float ds_f = (float)ds;
  if (!(ds >= 0.0) || !(ds_f >= 0.0f) || ds_f == __builtin_inff()) return REGNET_ERR_UNSUPPORTED;   // negative, NaN or infinite
  const GraspBox box{x_lo, x_hi, half_thickness, half_width, half_space, back_x};
  status = lattice_call_tail(&call, box, 0.0f, x_extent, B, origin3, field && L && dirs && result);
  if (status != REGNET_OK || B == 0) return status;
  const Fan fan{(int)R, (int)K, ds_f, thresh, dirs_grasp_stride};
  hipLaunchKernelGGL(retreat_fan_kernel<SIGNED>, dim3((unsigned)(B * R)), dim3(HL_T), 0, as_stream(stream), field, call.grid,
                     outside, L, box, x_hi_per_grasp, call.lat, dirs, fan, profile, result);
  REGNET_LAUNCH_CHECK();
  return REGNET_OK;
}

}  // namespace

extern "C" int regnet_grasp_retreat_fan_f32(const int32_t* field, int64_t nx, int64_t ny, int64_t nz, const float* origin3,
                                            double voxel, int outside, const float* L, int64_t B, float x_lo, float x_hi,
                                            const float* x_hi_per_grasp, float half_thickness, float half_width, float half_space,
                                            float back_x, double step, float x_extent, const float* dirs,
                                            int64_t dirs_grasp_stride, int64_t R, int64_t K, double ds, int thresh,
                                            int32_t* profile, int32_t* result, void* stream) {
  return retreat_fan<false>(field, nx, ny, nz, origin3, voxel, outside, L, B, x_lo, x_hi, x_hi_per_grasp, half_thickness,
                            half_width, half_space, back_x, step, x_extent, dirs, dirs_grasp_stride, R, K, ds, thresh, profile,
                            result, stream);
}

extern "C" int regnet_grasp_retreat_fan_signed_f32(const int32_t* field, int64_t nx, int64_t ny, int64_t nz, const float* origin3,
                                                   double voxel, int outside, const float* L, int64_t B, float x_lo, float x_hi,
                                                   const float* x_hi_per_grasp, float half_thickness, float half_width,
                                                   float half_space, float back_x, double step, float x_extent, const float* dirs,
                                                   int64_t dirs_grasp_stride, int64_t R, int64_t K, double ds, int thresh,
                                                   int32_t* profile, int32_t* result, void* stream) {
  return retreat_fan<true>(field, nx, ny, nz, origin3, voxel, outside, L, B, x_lo, x_hi, x_hi_per_grasp, half_thickness,
                           half_width, half_space, back_x, step, x_extent, dirs, dirs_grasp_stride, R, K, ds, thresh, profile,
                           result, stream);
}

extern "C" int regnet_grasp_retreat_pick(const int32_t* result, int64_t B, int64_t R, int32_t* best, void* stream) {
  if (B < 0 || R < 1) return REGNET_ERR_SHAPE;
  if (R > HF_MAX_R || B >= (int64_t)1 << 31) return REGNET_ERR_UNSUPPORTED;
  if (B == 0) return REGNET_OK;
  if (!result || !best) return REGNET_ERR_NULL;
  hipLaunchKernelGGL(retreat_pick_kernel, dim3((unsigned)((B + HL_T - 1) / HL_T)), dim3(HL_T), 0, as_stream(stream), result, B,
                     (int)R, best);
  REGNET_LAUNCH_CHECK();
  return REGNET_OK;
}
