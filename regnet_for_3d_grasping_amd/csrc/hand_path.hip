// hand_path.hip -- hand paths (include/regnet_hip.h "hand paths"): the rigid hand taken through K + 1 POSES per candidate path,
// read against the distance field at every waypoint.  The retreat fan (retreat.hip) translates the hand at its final pose; here
// the pose differs at every step, so a path may turn the wrist as it backs out.
//
// One workgroup of HL_T threads per (grasp, path), as in retreat_fan_kernel.  The (K + 1) x 12 rows of the path are staged in LDS
// once (at most 3 120 bytes); in the walk every lane reads the same row, a broadcast.  A thread decides a sample's membership once
// and then runs the K + 1 waypoints of that sample.  The per-waypoint minima live in LDS, lowered by a read-before-atomicMin: the
// word only ever falls, so a stale read costs an atomic and never a result.  The OUTSIDE count is one register per thread, summed
// by the wave butterfly and the four waves through LDS.  After one barrier threads 0..K store the profile, threads 0..K-1 compute
// the displacement between two waypoints and thread 0 walks the prefix.  Integer work only past the lookup: two runs give the same
// bytes.  result's layout is the fan's, so regnet_grasp_retreat_pick picks from it unchanged.
#include "hand_lattice.h"

namespace {

constexpr int HP_MAX_R = 16;
constexpr int HP_MAX_K = 64;
constexpr int HP_NONE = REGNET_EDT_NONE;

// one waypoint's rows applied to a point: grasp_apply with the rows read from LDS
__device__ __forceinline__ void rows_apply(const float* rows, float px, float py, float pz, float& x, float& y, float& z) {
  x = affine3(rows, px, py, pz);
  y = affine3(rows + 4, px, py, pz);
  z = affine3(rows + 8, px, py, pz);
}

template <bool SIGNED>
__global__ __launch_bounds__(HL_T) void hand_path_kernel(const int32_t* __restrict__ field, VoxelGrid grid, int outside,
                                                         const float* __restrict__ P, int R, int K, GraspBox box,
                                                         const float* __restrict__ x_hi_per_grasp, Lattice lat, int thresh,
                                                         int32_t* __restrict__ profile, int32_t* __restrict__ result,
                                                         float* __restrict__ disp) {
  __shared__ float rows[(HP_MAX_K + 1) * 12];
  __shared__ int step_min[HP_MAX_K + 1];
  __shared__ int red_out[HL_W];
  const int64_t pair = blockIdx.x;                   // (b, r), r fastest
  const int64_t b = pair / R;
  const int n_rows = (K + 1) * 12;
  const float* path = P + pair * n_rows;
  for (int i = threadIdx.x; i < n_rows; i += HL_T) rows[i] = path[i];
  for (int k = threadIdx.x; k <= K; k += HL_T) step_min[k] = HP_NONE;
  const float x_hi = x_hi_per_grasp ? x_hi_per_grasp[b] : box.x_hi;
  int n_out = 0;
  __syncthreads();
  lattice_walk(lat, box, x_hi, [&](float x, float y, float z, const HandSets& in) {
    if (!(in.back || in.finger)) return;             // the hand alone; membership is decided once, in the local frame
    for (int k = 0; k <= K; ++k) {
      float wx, wy, wz;
      rows_apply(rows + k * 12, x, y, z, wx, wy, wz);
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
  const int t = threadIdx.x;                         // (K + 1 <= 65 < HL_T: one waypoint per thread)
  if (profile && t <= K) profile[pair * (K + 1) + t] = step_min[t];
  if (disp && t < K) {
    // the largest distance a corner of the hand's bounding box moves from waypoint t to t + 1; the maximum over the corners is
    // the maximum over the box (DESIGN.md "Hand paths")
    const float* a = rows + t * 12;
    const float* c = a + 12;
    float far = 0.0f;
#pragma unroll
    for (int corner = 0; corner < 8; ++corner) {
      const float px = (corner & 1) ? x_hi : box.x_lo;
      const float py = (corner & 2) ? box.half_width : -box.half_width;
      const float pz = (corner & 4) ? box.half_thickness : -box.half_thickness;
      float ax, ay, az, cx, cy, cz;
      rows_apply(a, px, py, pz, ax, ay, az);
      rows_apply(c, px, py, pz, cx, cy, cz);
      const float dx = cx - ax, dy = cy - ay, dz = cz - az;
      // the contract asks for a correctly rounded float32 root: that is sqrtf here, and NOT __fsqrt_rn, which this toolchain
      // lowers to the native approximation (as tsdf.hip and depth.hip note)
      far = max_nan(far, sqrtf(dot3(dx, dy, dz, dx, dy, dz)));
    }
    disp[pair * K + t] = far;
  }
  if (t == 0) {
    int free_steps = 0, free_min = HP_NONE, all_min = HP_NONE;
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

template <bool SIGNED>
int hand_path(const int32_t* field, int64_t nx, int64_t ny, int64_t nz, const float* origin3, double voxel, int outside,
              const float* P, int64_t B, int64_t R, int64_t K, float x_lo, float x_hi, const float* x_hi_per_grasp,
              float half_thickness, float half_width, float half_space, float back_x, double step, float x_extent, int thresh,
              int32_t* profile, int32_t* result, float* disp, void* stream) {
  if (B < 0 || outside < 0 || outside > 1 || R < 1 || K < 1) return REGNET_ERR_SHAPE;
  const int dims = field_dims(nx, ny, nz);
  if (dims != REGNET_OK) return dims;
  if (B >= (int64_t)1 << 31) return REGNET_ERR_UNSUPPORTED;
  float voxel_f, h;
  if (!positive_f32(voxel, &voxel_f) || !positive_f32(step, &h)) return REGNET_ERR_UNSUPPORTED;
  if (R > HP_MAX_R || K > HP_MAX_K || B * R * (K + 1) > ((int64_t)1 << 28)) return REGNET_ERR_UNSUPPORTED;
  Lattice lat;
  if (!lattice_of(x_lo, 0.0f, half_thickness, half_width, x_extent, h, &lat)) return REGNET_ERR_UNSUPPORTED;
  if (B == 0) return REGNET_OK;
  if (!field || !origin3 || !P || !result) return REGNET_ERR_NULL;
  const VoxelGrid grid{(int)nx, (int)ny, (int)nz, origin3[0], origin3[1], origin3[2], voxel_f};
  const GraspBox box{x_lo, x_hi, half_thickness, half_width, half_space, back_x};
  hipLaunchKernelGGL(hand_path_kernel<SIGNED>, dim3((unsigned)(B * R)), dim3(HL_T), 0, as_stream(stream), field, grid, outside, P,
                     (int)R, (int)K, box, x_hi_per_grasp, lat, thresh, profile, result, disp);
  REGNET_LAUNCH_CHECK();
  return REGNET_OK;
}

}  // namespace

extern "C" int regnet_grasp_path_check_f32(const int32_t* field, int64_t nx, int64_t ny, int64_t nz, const float* origin3,
                                           double voxel, int outside, const float* P, int64_t B, int64_t R, int64_t K, float x_lo,
                                           float x_hi, const float* x_hi_per_grasp, float half_thickness, float half_width,
                                           float half_space, float back_x, double step, float x_extent, int thresh,
                                           int32_t* profile, int32_t* result, float* disp, void* stream) {
  return hand_path<false>(field, nx, ny, nz, origin3, voxel, outside, P, B, R, K, x_lo, x_hi, x_hi_per_grasp, half_thickness,
                          half_width, half_space, back_x, step, x_extent, thresh, profile, result, disp, stream);
}

extern "C" int regnet_grasp_path_check_signed_f32(const int32_t* field, int64_t nx, int64_t ny, int64_t nz, const float* origin3,
                                                  double voxel, int outside, const float* P, int64_t B, int64_t R, int64_t K,
                                                  float x_lo, float x_hi, const float* x_hi_per_grasp, float half_thickness,
                                                  float half_width, float half_space, float back_x, double step, float x_extent,
                                                  int thresh, int32_t* profile, int32_t* result, float* disp, void* stream) {
  return hand_path<true>(field, nx, ny, nz, origin3, voxel, outside, P, B, R, K, x_lo, x_hi, x_hi_per_grasp, half_thickness,
                         half_width, half_space, back_x, step, x_extent, thresh, profile, result, disp, stream);
}
