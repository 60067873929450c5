// view_gain.hip -- next-best view on the device (gfx950): which candidate camera pose reveals the most of the space no view has
// observed yet.  include/regnet_hip.h ("next-best view") is the contract; tests/view_gain_reference.py restates it in numpy.
//
//   * view_mark_kernel: grid z is the candidate pose, a lane a pixel of its coarse virtual camera.  The ray is the raycast's (tsdf.hip:
//     the same depths, deprojection and product with the pose), the lookup and the class are approach_volume.hip's (hand_lattice.h:
//     the NEAREST voxel; OUTSIDE / UNKNOWN / SOLID / FREE).  Every UNKNOWN voxel the ray reaches before a SOLID one, or before it has
//     crossed max_unknown unknown samples, gets bit `pose` of its word of the plane: an integer atomic OR, skipped when a plain load
//     shows the bit already set (bits are only ever set during the launch, so a stale load can only cost the atomic, never a bit).
//     A workgroup is 16 x 16 pixels and a wave an 8 x 8 tile, so a wave's 64 rays stay in neighbouring voxels.
//   * view_count_kernel / view_decide_kernel: the greedy joint pick.  Per round a pass over the plane counts, per pose, the words
//     with its bit set and no bit of a chosen pose (wave ballots and population counts into scalars; a wave whose words are all
//     zero or covered is skipped), and one workgroup picks the largest count, the lowest index on a tie, and adds it to the chosen
//     mask in a small device state block.  Integer sums only: the order of the reduction is free.
//   * view_interest_kernel: approach_volume.hip's lattice of the swept hand, one workgroup per grasp; every looked-up sample whose
//     voxel is UNKNOWN stores 1 into the interest plane (the same byte from every writer: no atomic).
//
// Canonical fp32: individually rounded operations in the written order (-ffp-contract=off), __fdiv_rn, strict comparisons.  The
// volume is only read.  No host read, no synchronisation, no allocation, no floating-point atomic: capturable.
#include "hand_lattice.h"
#include "ray_clip.h"

namespace {

constexpr int VG_T = 256;
constexpr int VG_TILE = 8, VG_WX = 2, VG_WY = 2;    // a wave is an 8 x 8 pixel tile, a workgroup 2 x 2 of them (the raycast's)
constexpr int VG_MAX_STEPS = 4096, VG_MAX_POSES = 32;
constexpr int VG_MAX_DIM = 1 << 24;
constexpr int64_t VG_MAX_VOXELS = (int64_t)1 << 28, VG_MAX_PIXELS = (int64_t)1 << 21;
constexpr int VG_COUNT_GROUPS = 2048;               // the counting pass's grid at most: 8 workgroups per CU in flight, then a stride
constexpr int VG_STATE_WORDS = REGNET_VIEW_PICK_STATE_WORDS;

enum { VG_EXITED = 0, VG_BLOCKED = 1, VG_SATURATED = 2, VG_REQUESTED = 3, VG_COLUMNS = 4 };
enum { VG_CHOSEN = 0, VG_STOPPED = 1, VG_COUNTS = 2 };      // the state block: the chosen mask, the stop flag, 32 counts

struct MarkArgs {
  VolumeView vol;
  int n_steps, width, height, clip, max_unknown;
  float rfx, rfy, cx, cy;
  float near, step;
};

// the fills of the entry points: n words of `value`, a grid stride (a kernel and not a memset, so that a captured call is kernel
// nodes only)
__global__ __launch_bounds__(VG_T) void view_fill_kernel(uint32_t* __restrict__ words, int n, uint32_t value) {
  const int stride = (int)gridDim.x * VG_T;
  for (int l = (int)blockIdx.x * VG_T + (int)threadIdx.x; l < n; l += stride) words[l] = value;      // n <= 2^28, stride <= 2^19
}

__global__ __launch_bounds__(VG_T) void view_mark_kernel(const MarkArgs a, const float* __restrict__ poses,
                                                         const uint8_t* __restrict__ interest, uint32_t* plane,
                                                         uint8_t* __restrict__ status, int32_t* __restrict__ rays) {
  __shared__ int s_hist[VG_COLUMNS];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int pose = (int)blockIdx.z;
  const int tiles_x = (a.width + VG_TILE * VG_WX - 1) / (VG_TILE * VG_WX);
  const int bx = (int)(blockIdx.x % (unsigned)tiles_x), by = (int)(blockIdx.x / (unsigned)tiles_x);
  const int u = (bx * VG_WX + (wave % VG_WX)) * VG_TILE + (lane & (VG_TILE - 1));
  const int v = (by * VG_WY + (wave / VG_WX)) * VG_TILE + (lane / VG_TILE);
  const bool active = u < a.width && v < a.height;
  if (tid < VG_COLUMNS) s_hist[tid] = 0;
  __syncthreads();
  float r[12];
#pragma unroll
  for (int k = 0; k < 12; ++k) r[k] = poses[(int64_t)pose * 12 + k];
  const uint32_t bit = 1u << pose;
  int code = VG_EXITED;
  bool requested = false;
  if (active) {
    const float du = (float)u - a.cx, dv = (float)v - a.cy;
    int first = 0, last = a.n_steps - 1;
    if (a.clip) {
      const int n[3] = {a.vol.grid.nx, a.vol.grid.ny, a.vol.grid.nz};
      const float o[3] = {a.vol.grid.ox, a.vol.grid.oy, a.vol.grid.oz};
      ray_clip(r, n, o, a.vol.grid.voxel, a.near, a.step, a.n_steps, du, dv, a.rfx, a.rfy, first, last);
    }
    int unknown = 0;
    int64_t seen = -1;                               // the voxel of the last inside sample, and its class: the volume does not change
    VoxelClass cls = VC_OUTSIDE;
    bool wanted = false;
    for (int i = first; i <= last; ++i) {
      const float z = a.near + ((float)i * a.step);
      const float cx = (du * z) * a.rfx, cy = (dv * z) * a.rfy;
      const float wx = affine3(r, cx, cy, z), wy = affine3(r + 4, cx, cy, z), wz = affine3(r + 8, cx, cy, z);
      int64_t l;
      if (!grid_voxel(a.vol.grid, wx, wy, wz, l)) continue;      // OUTSIDE
      if (l != seen) {
        seen = l;
        cls = voxel_class(a.vol, true, l);
        wanted = cls == VC_UNKNOWN && (interest == nullptr || interest[l] != 0);
        if (wanted && (plane[l] & bit) == 0u) atomicOr(&plane[l], bit);
      }
      if (cls == VC_SOLID) { code = VG_BLOCKED; break; }
      if (cls == VC_UNKNOWN) {
        requested = requested || wanted;
        if (++unknown == a.max_unknown) { code = VG_SATURATED; break; }
      }
    }
    if (status) status[((int64_t)pose * a.height + v) * a.width + u] = (uint8_t)code;
  }
#pragma unroll
  for (int c = 0; c < VG_COLUMNS; ++c) {
    const bool mine = active && (c == VG_REQUESTED ? requested : code == c);
    const int n = __popcll(__ballot(mine));
    if (lane == 0 && n != 0) atomicAdd(&s_hist[c], n);
  }
  __syncthreads();
  if (tid < VG_COLUMNS) {                            // one integer atomic per workgroup and column
    const int n = s_hist[tid];
    if (n != 0) atomicAdd(&rays[pose * VG_COLUMNS + tid], n);
  }
}

// per pose p < P: state[VG_COUNTS + p] += the words of the plane with bit p set and no bit of state[VG_CHOSEN]
__global__ __launch_bounds__(VG_T) void view_count_kernel(const uint32_t* __restrict__ plane, int n, int P, int32_t* state) {
  __shared__ int s_count[VG_MAX_POSES];
  const int tid = threadIdx.x, lane = tid & 63;
  if (tid < VG_MAX_POSES) s_count[tid] = 0;
  __syncthreads();
  const uint32_t chosen = (uint32_t)state[VG_CHOSEN];
  int count[VG_MAX_POSES];                           // wave-uniform: scalars
#pragma unroll
  for (int p = 0; p < VG_MAX_POSES; ++p) count[p] = 0;
  const int stride = (int)gridDim.x * VG_T;          // n <= 2^28 and stride <= 2^19: base + tid < 2^31
  for (int base = (int)blockIdx.x * VG_T; base < n; base += stride) {
    const int l = base + tid;
    uint32_t w = l < n ? plane[l] : 0u;
    if (w & chosen) w = 0u;
    if (__ballot(w != 0u) == 0ull) continue;         // most of the plane is zero
#pragma unroll
    for (int p = 0; p < VG_MAX_POSES; ++p) {
      if (p < P) count[p] += (int)__popcll(__ballot((w >> p) & 1u));
    }
  }
#pragma unroll
  for (int p = 0; p < VG_MAX_POSES; ++p) {
    if (lane == 0 && count[p] != 0) atomicAdd(&s_count[p], count[p]);
  }
  __syncthreads();
  if (tid < P) {
    const int c = s_count[tid];
    if (c != 0) atomicAdd(&state[VG_COUNTS + tid], c);
  }
}

// round r of the greedy pick: one wave.  Reads the round's counts, writes order[r] / order_gain[r] (and gain in round 0, where
// nothing is chosen yet), adds the winner to the chosen mask and clears the counts for the next round.
__global__ __launch_bounds__(64) void view_decide_kernel(int32_t* state, int P, int round, int floor_gain, int32_t* __restrict__ gain,
                                                         int32_t* __restrict__ order, int32_t* __restrict__ order_gain) {
  const int lane = (int)threadIdx.x;
  const int c = lane < P ? state[VG_COUNTS + lane] : 0;
  if (round == 0 && lane < P) gain[lane] = c;
  // the largest count, the lowest index among equals: the maximum of (count, 63 - lane)
  long long key = lane < P ? (((long long)c << 6) | (long long)(63 - lane)) : -1ll;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const long long other = __shfl_xor(key, o);
    key = other > key ? other : key;
  }
  const int stopped = state[VG_STOPPED];
  __syncthreads();                                   // every lane has read the state block before lane 0 and the clears write it
  if (lane < P) state[VG_COUNTS + lane] = 0;
  if (lane == 0) {
    const int best = (int)(key >> 6), winner = 63 - (int)(key & 63);
    if (stopped != 0 || best < floor_gain) {
      state[VG_STOPPED] = 1;
      order[round] = -1;
      order_gain[round] = 0;
    } else {
      state[VG_CHOSEN] = (int32_t)((uint32_t)state[VG_CHOSEN] | (1u << winner));
      order[round] = winner;
      order_gain[round] = best;
    }
  }
}

__global__ __launch_bounds__(HL_T) void view_interest_kernel(VolumeView vol, const float* __restrict__ L, GraspBox box,
                                                             const float* __restrict__ x_hi_per_grasp, Lattice lat,
                                                             uint8_t* __restrict__ interest, int32_t* __restrict__ counts) {
  __shared__ int red[HL_W];
  const GraspRows g = grasp_rows(L, blockIdx.x, 12);
  const float x_hi = x_hi_per_grasp ? x_hi_per_grasp[blockIdx.x] : box.x_hi;
  int unknown = 0;
  lattice_walk(lat, box, x_hi, [&](float x, float y, float z, const HandSets& in) {
    if (!(in.region || in.back || in.finger || in.blocker)) return;      // in no set: no lookup
    float wx, wy, wz;
    grasp_apply(g, x, y, z, wx, wy, wz);
    int64_t v;
    const bool inside = grid_voxel(vol.grid, wx, wy, wz, v);
    if (voxel_class(vol, inside, v) != VC_UNKNOWN) return;
    interest[v] = 1;
    unknown += 1;
  });
  unknown = wave_sum(unknown);
  block_put(unknown, red);
  __syncthreads();
  if (threadIdx.x == 0) counts[blockIdx.x] = block_sum<HL_W>(red);
}

// the checks every entry point that reads the volume shares: REGNET_OK, or the status of the first rule broken
int volume_shape(int64_t nx, int64_t ny, int64_t nz, int64_t min_weight) {
  return (nx < 1 || ny < 1 || nz < 1 || min_weight < 1) ? REGNET_ERR_SHAPE : REGNET_OK;
}
bool volume_supported(int64_t nx, int64_t ny, int64_t nz, int64_t min_weight, double voxel, double trunc, double margin,
                      float* voxel_f, float* d_solid) {
  if (nx > VG_MAX_DIM || ny > VG_MAX_DIM || nz > VG_MAX_DIM || nx * ny * nz > VG_MAX_VOXELS) return false;
  if (min_weight >= (int64_t)1 << 31) return false;
  float trunc_f;
  if (!positive_f32(voxel, voxel_f) || !positive_f32(trunc, &trunc_f)) return false;
  *d_solid = (float)(margin / trunc);
  return *d_solid == *d_solid && *d_solid != __builtin_inff() && *d_solid != -__builtin_inff();
}

unsigned fill_grid(int64_t n) {
  const int64_t groups = (n + VG_T - 1) / VG_T;
  return (unsigned)(groups < VG_COUNT_GROUPS ? groups : VG_COUNT_GROUPS);
}

VolumeView view_of(const void* volume, int64_t nx, int64_t ny, int64_t nz, const float* origin3, float voxel_f, float d_solid,
                   int64_t min_weight) {
  const Planes planes = planes_of(const_cast<void*>(volume), nx * ny * nz);
  return VolumeView{planes.D, planes.W, VoxelGrid{(int)nx, (int)ny, (int)nz, origin3[0], origin3[1], origin3[2], voxel_f}, d_solid,
                    (int)min_weight};
}

}  // namespace

extern "C" int regnet_tsdf_view_mark_f32(const void* volume, int64_t nx, int64_t ny, int64_t nz, const float* origin3, double voxel,
                                         double trunc, int64_t min_weight, double margin, const float* intrinsics4,
                                         const float* poses, int64_t P, double near, double step, int64_t n_steps, int64_t width,
                                         int64_t height, int clip, int64_t max_unknown, const uint8_t* interest, uint32_t* plane,
                                         uint8_t* status, int32_t* rays, void* stream) {
  if (volume_shape(nx, ny, nz, min_weight) != REGNET_OK || P < 1 || width < 1 || height < 1 || n_steps < 1 || max_unknown < 1)
    return REGNET_ERR_SHAPE;
  float voxel_f, d_solid, near_f, step_f;
  if (!volume_supported(nx, ny, nz, min_weight, voxel, trunc, margin, &voxel_f, &d_solid)) return REGNET_ERR_UNSUPPORTED;
  if (P > VG_MAX_POSES || n_steps > VG_MAX_STEPS || max_unknown > n_steps) return REGNET_ERR_UNSUPPORTED;
  if (width > VG_MAX_PIXELS || height > VG_MAX_PIXELS || width * height > VG_MAX_PIXELS) return REGNET_ERR_UNSUPPORTED;
  if (!positive_f32(near, &near_f) || !positive_f32(step, &step_f)) return REGNET_ERR_UNSUPPORTED;
  if (!volume || !origin3 || !intrinsics4 || !poses || !plane || !rays) return REGNET_ERR_NULL;
  MarkArgs a;
  a.vol = view_of(volume, nx, ny, nz, origin3, voxel_f, d_solid, min_weight);
  a.n_steps = (int)n_steps; a.width = (int)width; a.height = (int)height; a.clip = clip != 0; a.max_unknown = (int)max_unknown;
  a.rfx = intrinsics4[0]; a.rfy = intrinsics4[1]; a.cx = intrinsics4[2]; a.cy = intrinsics4[3];
  a.near = near_f; a.step = step_f;
  hipStream_t s = as_stream(stream);
  const int64_t n = nx * ny * nz;
  hipLaunchKernelGGL(view_fill_kernel, dim3(fill_grid(n)), dim3(VG_T), 0, s, plane, (int)n, 0u);
  REGNET_LAUNCH_CHECK();
  hipLaunchKernelGGL(view_fill_kernel, dim3(1), dim3(VG_T), 0, s, (uint32_t*)rays, (int)P * VG_COLUMNS, 0u);
  REGNET_LAUNCH_CHECK();
  const int64_t tiles = ((width + VG_TILE * VG_WX - 1) / (VG_TILE * VG_WX)) * ((height + VG_TILE * VG_WY - 1) / (VG_TILE * VG_WY));
  hipLaunchKernelGGL(view_mark_kernel, dim3((unsigned)tiles, 1, (unsigned)P), dim3(VG_T), 0, s, a, poses, interest, plane, status,
                     rays);
  REGNET_LAUNCH_CHECK();
  return REGNET_OK;
}

extern "C" int regnet_tsdf_view_pick(const uint32_t* plane, int64_t N, int64_t P, int64_t K, int64_t min_gain, int32_t* state,
                                     int32_t* gain, int32_t* order, int32_t* order_gain, void* stream) {
  if (N < 1 || P < 1 || K < 1 || min_gain < 0) return REGNET_ERR_SHAPE;
  if (N > VG_MAX_VOXELS || P > VG_MAX_POSES || K > P) return REGNET_ERR_UNSUPPORTED;
  if (!plane || !state || !gain || !order || !order_gain) return REGNET_ERR_NULL;
  const int floor_gain = (int)(min_gain < 1 ? 1 : (min_gain > 0x7FFFFFFF ? 0x7FFFFFFF : min_gain));
  hipStream_t s = as_stream(stream);
  hipLaunchKernelGGL(view_fill_kernel, dim3(1), dim3(VG_T), 0, s, (uint32_t*)state, VG_STATE_WORDS, 0u);
  REGNET_LAUNCH_CHECK();
  const unsigned grid = fill_grid(N);
  for (int round = 0; round < (int)K; ++round) {
    hipLaunchKernelGGL(view_count_kernel, dim3(grid), dim3(VG_T), 0, s, plane, (int)N, (int)P, state);
    REGNET_LAUNCH_CHECK();
    hipLaunchKernelGGL(view_decide_kernel, dim3(1), dim3(64), 0, s, state, (int)P, round, floor_gain, gain, order, order_gain);
    REGNET_LAUNCH_CHECK();
  }
  return REGNET_OK;
}

extern "C" int regnet_tsdf_view_interest_hands(const void* volume, int64_t nx, int64_t ny, int64_t nz, const float* origin3,
                                               double voxel, double trunc, int64_t min_weight, double margin, const float* L,
                                               int64_t B, float x_lo, float x_hi, const float* x_hi_per_grasp,
                                               float half_thickness, float half_width, float half_space, float back_x,
                                               float standoff, double step, float x_extent, uint8_t* interest, int32_t* counts,
                                               void* stream) {
  if (B < 0 || volume_shape(nx, ny, nz, min_weight) != REGNET_OK) return REGNET_ERR_SHAPE;
  float voxel_f, d_solid, h;
  if (!volume_supported(nx, ny, nz, min_weight, voxel, trunc, margin, &voxel_f, &d_solid)) return REGNET_ERR_UNSUPPORTED;
  if (B >= (int64_t)1 << 31 || !positive_f32(step, &h)) return REGNET_ERR_UNSUPPORTED;
  LatticeCall call{VoxelGrid{}, Lattice{}, h};       // (the grid is view_of's)
  const GraspBox box{x_lo, x_hi, half_thickness, half_width, half_space, back_x};
  const int status = lattice_call_tail(&call, box, standoff, x_extent, B, origin3, volume && L && interest && counts);
  if (status != REGNET_OK || B == 0) return status;
  hipLaunchKernelGGL(view_interest_kernel, dim3((unsigned)B), dim3(HL_T), 0, as_stream(stream),
                     view_of(volume, nx, ny, nz, origin3, voxel_f, d_solid, min_weight), L, box, x_hi_per_grasp, call.lat, interest,
                     counts);
  REGNET_LAUNCH_CHECK();
  return REGNET_OK;
}
