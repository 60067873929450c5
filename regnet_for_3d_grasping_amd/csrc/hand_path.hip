// hand_path.hip -- hand paths (include/regnet_hip.h "hand paths"): the rigid hand taken through K + 1 POSES per candidate path,
// read against the distance field at every waypoint.  The retreat fan (retreat.hip) translates the hand at its final pose; here
// the pose differs at every step, so a path may turn the wrist as it backs out.
//
// One workgroup of HL_T threads per (grasp, path), the body hand_field.h's hand_steps, as in retreat_fan_kernel.  The (K + 1) x 12
// rows of the path are staged in LDS once (at most 3 120 bytes); in the walk every lane reads the same row, a broadcast.  After
// the body threads 0..K-1 compute the displacement between two waypoints.  result's layout is the fan's, so
// regnet_grasp_retreat_pick picks from it unchanged.
#include "hand_field.h"

namespace {

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
  __shared__ float rows[(HF_MAX_K + 1) * 12];
  const int64_t pair = blockIdx.x;                   // (b, r), r fastest
  const int64_t b = pair / R;
  const int n_rows = (K + 1) * 12;
  const float* path = P + pair * n_rows;
  for (int i = threadIdx.x; i < n_rows; i += HL_T) rows[i] = path[i];
  const float x_hi = x_hi_per_grasp ? x_hi_per_grasp[b] : box.x_hi;
  hand_steps<SIGNED>(field, grid, outside, box, x_hi, lat, K, thresh, pair, profile, result,
                     [&](int k, float x, float y, float z, float& wx, float& wy, float& wz) {
    rows_apply(rows + k * 12, x, y, z, wx, wy, wz);
  });
  const int t = threadIdx.x;                         // (K < HL_T: one displacement per thread)
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
}

template <bool SIGNED>
int hand_path(const int32_t* field, int64_t nx, int64_t ny, int64_t nz, const float* origin3, double voxel, int outside,
              const float* P, int64_t B, int64_t R, int64_t K, float x_lo, float x_hi, const float* x_hi_per_grasp,
              float half_thickness, float half_width, float half_space, float back_x, double step, float x_extent, int thresh,
              int32_t* profile, int32_t* result, float* disp, void* stream) {
  if (R < 1 || K < 1) return REGNET_ERR_SHAPE;       // (with the opening checks' own SHAPE rules: one status)
  LatticeCall call;
  int status = field_call_checks(nx, ny, nz, voxel, outside, B, step, &call);
  if (status != REGNET_OK) return status;
  if (R > HF_MAX_R || K > HF_MAX_K || B * R * (K + 1) > ((int64_t)1 << 28)) return REGNET_ERR_UNSUPPORTED;
  const GraspBox box{x_lo, x_hi, half_thickness, half_width, half_space, back_x};
  status = lattice_call_tail(&call, box, 0.0f, x_extent, B, origin3, field && P && result);
  if (status != REGNET_OK || B == 0) return status;
  hipLaunchKernelGGL(hand_path_kernel<SIGNED>, dim3((unsigned)(B * R)), dim3(HL_T), 0, as_stream(stream), field, call.grid,
                     outside, P, (int)R, (int)K, box, x_hi_per_grasp, call.lat, thresh, profile, result, disp);
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
