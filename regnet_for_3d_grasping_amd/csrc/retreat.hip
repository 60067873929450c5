// retreat.hip -- the retreat fan (include/regnet_hip.h "retreat fan"): the rigid hand at its final pose, moved along R candidate
// directions in K steps and read against the distance field at every step, and the pick of the best direction per grasp.
//
// One workgroup of HL_T threads per (grasp, direction).  The lattice is the margin kernel's with standoff 0 and the walk is
// hand_lattice.h's: a thread decides a sample's membership once and then runs the K + 1 steps of that sample.  The per-step minima
// live in LDS, one word per step, not in registers: a thread compares its value with the word (a broadcast read) and issues the
// LDS integer min only when it would lower it -- the word only ever falls, so a stale read costs an atomic and never a result,
// and a minimum has no order.  The OUTSIDE count is one register per thread, summed by the wave butterfly and the four waves
// through LDS.  After one barrier the first K + 1 threads store the profile and thread 0 walks the prefix.  Integer work only past
// the lookup: two runs give the same bytes.
#include "hand_lattice.h"

namespace {

constexpr int RF_MAX_R = 16;
constexpr int RF_MAX_K = 64;
constexpr int RF_NONE = REGNET_EDT_NONE;

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
  __shared__ int step_min[RF_MAX_K + 1];
  __shared__ int red_out[HL_W];
  const int64_t pair = blockIdx.x;                   // (b, r), r fastest
  const int64_t b = pair / fan.R;
  const int r = (int)(pair - b * fan.R);
  const int K = fan.K;
  for (int k = threadIdx.x; k <= K; k += HL_T) step_min[k] = RF_NONE;
  const GraspRows g = grasp_rows(L, b, 12);
  const float x_hi = x_hi_per_grasp ? x_hi_per_grasp[b] : box.x_hi;
  const float* d = dirs + b * fan.dirs_grasp_stride + 3 * r;
  const float dx = d[0], dy = d[1], dz = d[2];
  const float ds = fan.ds;
  int n_out = 0;
  __syncthreads();
  lattice_walk(lat, box, x_hi, [&](float x, float y, float z, const HandSets& in) {
    if (!(in.back || in.finger)) return;             // only the hand at its final pose moves
    for (int k = 0; k <= K; ++k) {
      const float t = (float)k * ds;
      const float px = x + (t * dx), py = y + (t * dy), pz = z + (t * dz);
      float wx, wy, wz;
      grasp_apply(g, px, py, pz, wx, wy, wz);
      int64_t v;
      const bool inside = grid_voxel(grid, wx, wy, wz, v);
      if (!inside) {
        n_out += (int)(k > 0);
        if (!outside) continue;                      // skipped; else it lies in an obstacle: 0 (signed: -1)
      }
      const int value = inside ? field[v] : (SIGNED ? -1 : 0);
      if (value < step_min[k]) atomicMin(&step_min[k], value);
    }
  });
  n_out = wave_sum(n_out);
  block_put(n_out, red_out);
  __syncthreads();
  if (profile) {
    for (int k = threadIdx.x; k <= K; k += HL_T) profile[pair * (K + 1) + k] = step_min[k];
  }
  if (threadIdx.x == 0) {
    int free_steps = 0, free_min = RF_NONE, all_min = RF_NONE;
    bool open = true;
    for (int k = 1; k <= K; ++k) {
      const int m = step_min[k];
      all_min = min(all_min, m);
      open = open && m >= fan.thresh;
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
  if (B < 0 || outside < 0 || outside > 1 || R < 1 || K < 1 || dirs_grasp_stride < 0) return REGNET_ERR_SHAPE;
  const int dims = field_dims(nx, ny, nz);
  if (dims != REGNET_OK) return dims;
  if (B >= (int64_t)1 << 31) return REGNET_ERR_UNSUPPORTED;
  float voxel_f, h;
  if (!positive_f32(voxel, &voxel_f) || !positive_f32(step, &h)) return REGNET_ERR_UNSUPPORTED;
  if (R > RF_MAX_R || K > RF_MAX_K || B * R * (K + 1) > ((int64_t)1 << 28)) return REGNET_ERR_UNSUPPORTED;
  const float ds_f = (float)ds;
  if (!(ds >= 0.0) || !(ds_f >= 0.0f) || ds_f == __builtin_inff()) return REGNET_ERR_UNSUPPORTED;   // negative, NaN or infinite
  Lattice lat;
  if (!lattice_of(x_lo, 0.0f, half_thickness, half_width, x_extent, h, &lat)) return REGNET_ERR_UNSUPPORTED;
  if (B == 0) return REGNET_OK;
  if (!field || !origin3 || !L || !dirs || !result) return REGNET_ERR_NULL;
  const VoxelGrid grid{(int)nx, (int)ny, (int)nz, origin3[0], origin3[1], origin3[2], voxel_f};
  const GraspBox box{x_lo, x_hi, half_thickness, half_width, half_space, back_x};
  const Fan fan{(int)R, (int)K, ds_f, thresh, dirs_grasp_stride};
  hipLaunchKernelGGL(retreat_fan_kernel<SIGNED>, dim3((unsigned)(B * R)), dim3(HL_T), 0, as_stream(stream), field, grid, outside,
                     L, box, x_hi_per_grasp, lat, dirs, fan, profile, result);
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
  if (R > RF_MAX_R || B >= (int64_t)1 << 31) return REGNET_ERR_UNSUPPORTED;
  if (B == 0) return REGNET_OK;
  if (!result || !best) return REGNET_ERR_NULL;
  hipLaunchKernelGGL(retreat_pick_kernel, dim3((unsigned)((B + HL_T - 1) / HL_T)), dim3(HL_T), 0, as_stream(stream), result, B,
                     (int)R, best);
  REGNET_LAUNCH_CHECK();
  return REGNET_OK;
}
