// hand_adjust.hip -- the push-out (include/regnet_hip.h "push-out"): the rigid hand of every grasp moved by a TRANSLATION until its
// interpolated signed margin reaches a target.  The margin, the fan and the paths only judge a pose; this kernel follows the
// field's gradient out of a collision.  Deepest-sample projection: at every iterate the hand sample with the smallest
// interpolated signed distance is found, and the hand steps along the gradient there by the distance that is missing.
//
// One workgroup of HL_T threads per grasp, the whole iteration inside the kernel.  An iterate is one walk of the fan's lattice
// (hand_lattice.h): a thread reads the trilinear value of its hand samples (sdf_sample.h, eight loads each -- the hot loop) and
// keeps the smallest 64-bit key (ordered(value) << 32) | index in a register pair; the keys go through the wave butterfly and
// the four waves through LDS, in two sets of slots used in turn, so an iterate costs ONE barrier.  Every thread then holds the
// same key and takes the same decision: the exit is workgroup-uniform.  The gradient at the worst sample is recomputed by every
// thread from the key's index (the same eight addresses in every lane: a broadcast), which spares a second barrier.  The
// translation is recomputed from the accumulated LOCAL shift at every step, never accumulated in the volume's frame.  Integer
// minima and one integer sum only: two runs give the same bytes.
#include "sdf_sample.h"

namespace {

constexpr int PO_MAX_T = 64;
constexpr uint64_t PO_NO_KEY = ~(uint64_t)0;       // no sample has a value (a NaN is never keyed, so no key has these bits)

struct Push {
  float ax, ay, az;   // axes3
  float target, cap2;
  int T;
};

// the monotone map of float32 bits onto unsigned integers (-0 below +0) and back
__device__ __forceinline__ uint32_t ordered_bits(float v) {
  const int32_t b = __float_as_int(v);
  return (uint32_t)(b ^ ((b >> 31) | (int32_t)0x80000000));
}
__device__ __forceinline__ float ordered_value(uint32_t u) {
  return __uint_as_float((u & 0x80000000u) ? (u ^ 0x80000000u) : ~u);
}

__device__ __forceinline__ uint64_t wave_min_key(uint64_t key) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const uint32_t hi = (uint32_t)__shfl_xor((int)(key >> 32), o), lo = (uint32_t)__shfl_xor((int)(uint32_t)key, o);
    const uint64_t other = ((uint64_t)hi << 32) | lo;
    key = other < key ? other : key;
  }
  return key;
}

__global__ __launch_bounds__(HL_T) void push_out_kernel(const int32_t* __restrict__ field, VoxelGrid grid, int outside,
                                                        const float* __restrict__ L, GraspBox box,
                                                        const float* __restrict__ x_hi_per_grasp, Lattice lat, Push push,
                                                        float* __restrict__ pose, float* __restrict__ shift,
                                                        float* __restrict__ trace, int32_t* __restrict__ info) {
  __shared__ uint64_t red_key[2][HL_W];
  __shared__ int red_out[2][HL_W];
  __shared__ float minima[PO_MAX_T + 1];
  const int64_t b = blockIdx.x;
  const int tid = threadIdx.x;
  GraspRows g = grasp_rows(L, b, 12);               // rows 0..2; column 3 is rewritten at every applied step
  const float t0[3] = {g.r[0][3], g.r[1][3], g.r[2][3]};
  const float x_hi = x_hi_per_grasp ? x_hi_per_grasp[b] : box.x_hi;
  const int T = push.T;
  if (tid <= T) minima[tid] = __builtin_nanf("");   // (T + 1 <= 65 < HL_T)
  float s0 = 0.0f, s1 = 0.0f, s2 = 0.0f;
  int status, steps = 0, worst, n_out;
  for (int n = 0;; ++n) {
    uint64_t key = PO_NO_KEY;
    int out = 0;
    lattice_walk_at(lat, box, x_hi, [&](int i, int j, int k, float x, float y, float z, const HandSets& in) {
      if (!(in.back || in.finger)) return;           // the hand alone; membership is decided in the local frame
      float wx, wy, wz;
      grasp_apply(g, x, y, z, wx, wy, wz);
      int64_t v;
      float value = __builtin_nanf(""), u0, u1, u2;
      if (grid_voxel(grid, wx, wy, wz, v)) value = sdf_sample(field, grid, wx, wy, wz, false, u0, u1, u2);
      if (value != value) {                          // OUTSIDE, or a NaN value (infinite corners): no value, and counted
        out += 1;
        return;
      }
      const uint64_t mine = ((uint64_t)ordered_bits(value) << 32) | (uint32_t)((i * lat.ny + j) * lat.nz + k);
      key = mine < key ? mine : key;
    });
    key = wave_min_key(key);
    out = wave_sum(out);
    block_put(key, red_key[n & 1]);
    block_put(out, red_out[n & 1]);
    __syncthreads();                                 // (the other set of slots is written next: no second barrier)
    key = block_join<HL_W>(red_key[n & 1], [](uint64_t a, uint64_t c) { return a < c ? a : c; });
    n_out = block_sum<HL_W>(red_out[n & 1]);
    const bool valued = key != PO_NO_KEY;
    const float low = valued ? ordered_value((uint32_t)(key >> 32)) : __builtin_inff();
    worst = valued ? (int)(uint32_t)key : -1;
    if (tid == 0) minima[n] = low;
    if (!valued && n_out == 0) { status = REGNET_PUSH_ALREADY_FREE; break; }         // the hand has no sample
    if (!valued || (outside && n_out > 0)) { status = REGNET_PUSH_LEFT_VOLUME; break; }
    if (low >= push.target) { status = n == 0 ? REGNET_PUSH_ALREADY_FREE : REGNET_PUSH_FREED; break; }
    if (n == T) { status = REGNET_PUSH_MAX_ITER; break; }
    // the gradient at the worst sample, in the volume's frame (the sample was INSIDE; sdf_axis clamps every index anyway)
    const int k = worst % lat.nz, ij = worst / lat.nz, j = ij % lat.ny, i = ij / lat.ny;
    float x, y, z, wx, wy, wz, gx, gy, gz;
    lattice_point(lat, box, i, j, k, x, y, z);
    grasp_apply(g, x, y, z, wx, wy, wz);
    sdf_sample(field, grid, wx, wy, wz, true, gx, gy, gz);
    const float a0 = push.ax * dot3(g.r[0][0], g.r[1][0], g.r[2][0], gx, gy, gz);
    const float a1 = push.ay * dot3(g.r[0][1], g.r[1][1], g.r[2][1], gx, gy, gz);
    const float a2 = push.az * dot3(g.r[0][2], g.r[1][2], g.r[2][2], gx, gy, gz);
    const float e = push.target - low;
    const float d0 = e * a0, d1 = e * a1, d2 = e * a2;
    if (a0 != a0 || a1 != a1 || a2 != a2 || (d0 == 0.0f && d1 == 0.0f && d2 == 0.0f)) { status = REGNET_PUSH_STUCK; break; }
    const float c0 = s0 + d0, c1 = s1 + d1, c2 = s2 + d2;
    if (!(dot3(c0, c1, c2, c0, c1, c2) <= push.cap2)) { status = REGNET_PUSH_CAPPED; break; }   // (a NaN is capped too)
    s0 = c0; s1 = c1; s2 = c2;
    steps += 1;
#pragma unroll
    for (int r = 0; r < 3; ++r) g.r[r][3] = affine3(g.r[r][0], g.r[r][1], g.r[r][2], t0[r], s0, s1, s2);
  }
  __syncthreads();                                   // minima[] is complete (the exit above is workgroup-uniform)
  if (trace && tid <= T) trace[b * (T + 1) + tid] = minima[tid];
  if (tid == 0) {
#pragma unroll
    for (int w = 0; w < 12; ++w) pose[b * 12 + w] = g.r[w >> 2][w & 3];   // (static indices: the rows stay in registers)
    shift[b * 3] = s0; shift[b * 3 + 1] = s1; shift[b * 3 + 2] = s2;
    int32_t* o = info + b * 4;
    o[0] = status; o[1] = steps; o[2] = worst; o[3] = n_out;
  }
}

}  // namespace

extern "C" int regnet_grasp_push_out_f32(const int32_t* field, int64_t nx, int64_t ny, int64_t nz, const float* origin3,
                                         double voxel, int outside, const float* L, int64_t B, float x_lo, float x_hi,
                                         const float* x_hi_per_grasp, float half_thickness, float half_width, float half_space,
                                         float back_x, double step, float x_extent, const float* axes3, double target,
                                         double max_shift, int64_t T, float* pose, float* shift, float* trace, int32_t* info,
                                         void* stream) {
  if (T < 1) return REGNET_ERR_SHAPE;                // (with the opening checks' own SHAPE rules: one status)
  LatticeCall call;
  int status = field_call_checks(nx, ny, nz, voxel, outside, B, step, &call);
  if (status != REGNET_OK) return status;
  if (T > PO_MAX_T) return REGNET_ERR_UNSUPPORTED;
  const float target_f = (float)target, cap_f = (float)max_shift;
  if (!finite_f32(target_f) || !(max_shift >= 0.0) || !(cap_f >= 0.0f) || !finite_f32(cap_f)) return REGNET_ERR_UNSUPPORTED;
  if (axes3 && !(finite_f32(axes3[0]) && finite_f32(axes3[1]) && finite_f32(axes3[2]))) return REGNET_ERR_UNSUPPORTED;
  const GraspBox box{x_lo, x_hi, half_thickness, half_width, half_space, back_x};
  status = lattice_call_tail(&call, box, 0.0f, x_extent, B, origin3, field && L && axes3 && pose && shift && info);
  if (status != REGNET_OK || B == 0) return status;
  const Push push{axes3[0], axes3[1], axes3[2], target_f, cap_f * cap_f, (int)T};
  hipLaunchKernelGGL(push_out_kernel, dim3((unsigned)B), dim3(HL_T), 0, as_stream(stream), field, call.grid, outside, L, box,
                     x_hi_per_grasp, call.lat, push, pose, shift, trace, info);
  REGNET_LAUNCH_CHECK();
  return REGNET_OK;
}
