// approach_volume.hip -- per-grasp approach analysis against the TSDF volume on the device (gfx950): the swept hand is not held
// against the points some camera saw (approach.hip) but against the volume's three states per voxel -- seen solid, seen free,
// never observed -- so the occluded back of an object and the space no view reached can count as blocked.
//
// One workgroup of 256 threads per grasp.  Nothing is scanned but a LATTICE of samples of the swept hand in the grasp's local
// frame, shared by all grasps of a call: n_x x n_y x n_z cell-centred samples of step h over [x_lo - S, x_extent] x [-hw, hw] x
// [-ht, ht].  A wave takes 8 x 8 tiles of the lattice's x-y plane, tile t = wave, wave + 4, ..., lane l at (l & 7, l >> 3) of the
// tile, and walks the n_z layers: its 64 samples are neighbours in space, so their voxels are neighbours in the volume.  Every
// sample is taken into the volume's frame by the grasp's own L (rows 0..2 of a 4x4), looked up in the NEAREST voxel (one W, and
// one D when W >= min_weight) and classified; hand_box.h's sets, the ones approach.hip and region.hip use, say which it
// belongs to.  Canonical fp32: individually rounded operations in the written order (-ffp-contract=off), __fdiv_rn, strict
// comparisons.  Only integer sums and float min / max are reduced (common.h: the wave butterfly, then the waves through LDS): no atomic, no
// floating-point sum.  The volume is only read (tsdf_volume.h: its planes).  Plain vector stores by thread 0.  The lattice, its
// walk and the voxel lookup are hand_lattice.h's, which edt.hip's margin kernel shares.
#include "hand_lattice.h"

namespace {

constexpr int AV_T = HL_T;
constexpr int AV_W = HL_W;
constexpr int AV_NI = 8, AV_NF = 4;                  // reduced integers and floats

__global__ __launch_bounds__(AV_T) void approach_volume_kernel(VolumeView vol, const float* __restrict__ L, GraspBox box,
                                                               const float* __restrict__ x_hi_per_grasp, float standoff,
                                                               Lattice lat, int32_t* __restrict__ counts,
                                                               float* __restrict__ values) {
  __shared__ int red_i[AV_NI][AV_W];
  __shared__ float red_f[AV_NF][AV_W];
  const GraspRows g = grasp_rows(L, blockIdx.x, 12);
  const float x_hi = x_hi_per_grasp ? x_hi_per_grasp[blockIdx.x] : box.x_hi;

  int region_solid = 0, region_unseen = 0, hand_solid = 0, hand_unseen = 0, block_solid = 0, block_unseen = 0;
  int members = 0, members_outside = 0;
  float y_min = __builtin_inff(), y_max = -__builtin_inff(), s_seen = __builtin_inff(), s_safe = __builtin_inff();
  lattice_walk(lat, box, x_hi, [&](float x, float y, float z, const HandSets& in) {
    const bool region = in.region, blocker = in.blocker;
    const float s = in.retreat;
    const int hand = (int)in.back + (int)in.finger;
    const int member = hand + (int)blocker;
    if (!(region || member)) return;                 // in no set: no lookup
    float wx, wy, wz;
    grasp_apply(g, x, y, z, wx, wy, wz);
    int64_t v;
    const bool inside = grid_voxel(vol.grid, wx, wy, wz, v);
    const VoxelClass cls = voxel_class(vol, inside, v);
    const bool solid = cls == VC_SOLID, unseen = cls == VC_OUTSIDE || cls == VC_UNKNOWN;
    members += member;
    members_outside += inside ? 0 : member;
    if (solid) {
      hand_solid += hand;
      if (region) {
        region_solid += 1;
        y_min = fminf(y_min, y);
        y_max = fmaxf(y_max, y);
      }
      if (blocker) {
        block_solid += 1;
        s_seen = fminf(s_seen, s);
        s_safe = fminf(s_safe, s);
      }
    } else if (unseen) {
      hand_unseen += hand;
      region_unseen += (int)region;
      if (blocker) {
        block_unseen += 1;
        s_safe = fminf(s_safe, s);
      }
    }
  });
  int ri[AV_NI] = {region_solid, region_unseen, hand_solid, hand_unseen, block_solid, block_unseen, members, members_outside};
#pragma unroll
  for (int q = 0; q < AV_NI; ++q) ri[q] = wave_sum(ri[q]);
  y_min = wave_min(y_min); y_max = wave_max(y_max); s_seen = wave_min(s_seen); s_safe = wave_min(s_safe);
#pragma unroll
  for (int q = 0; q < AV_NI; ++q) block_put(ri[q], red_i[q]);
  block_put(y_min, red_f[0]); block_put(y_max, red_f[1]); block_put(s_seen, red_f[2]); block_put(s_safe, red_f[3]);
  __syncthreads();
  if (threadIdx.x == 0) {
    int32_t* c = counts + (int64_t)blockIdx.x * 8;
#pragma unroll
    for (int q = 0; q < AV_NI; ++q) c[q] = block_sum<AV_W>(red_i[q]);
    y_min = block_min<AV_W>(red_f[0]); y_max = block_max<AV_W>(red_f[1]);
    s_seen = block_min<AV_W>(red_f[2]); s_safe = block_min<AV_W>(red_f[3]);
    float* v = values + (int64_t)blockIdx.x * 4;
    v[0] = y_min + 0.0f; v[1] = y_max + 0.0f;        // (+ 0.0f: no -0.0 leaves the kernel)
    v[2] = fminf(standoff, s_seen) + 0.0f; v[3] = fminf(standoff, s_safe) + 0.0f;
  }
}

}  // namespace

extern "C" int regnet_grasp_approach_volume_f32(const void* volume, int64_t nx, int64_t ny, int64_t nz, const float* origin3,
                                                double voxel, double trunc, int64_t min_weight, double margin, const float* L,
                                                int64_t B, float x_lo, float x_hi, const float* x_hi_per_grasp,
                                                float half_thickness, float half_width, float half_space, float back_x,
                                                float standoff, double step, float x_extent, int32_t* counts, float* values,
                                                void* stream) {
  if (B < 0 || nx < 1 || ny < 1 || nz < 1 || min_weight < 1) return REGNET_ERR_SHAPE;
  const int64_t limit = (int64_t)1 << 24;             // (then (float)n is exact and the inside test compares exact floats)
  if (nx > limit || ny > limit || nz > limit || nx * ny * nz > ((int64_t)1 << 28)) return REGNET_ERR_UNSUPPORTED;
  if (B >= (int64_t)1 << 31 || min_weight >= (int64_t)1 << 31) return REGNET_ERR_UNSUPPORTED;
  float voxel_f, trunc_f, h;
  if (!positive_f32(voxel, &voxel_f) || !positive_f32(trunc, &trunc_f) || !positive_f32(step, &h)) return REGNET_ERR_UNSUPPORTED;
  const float d_solid = (float)(margin / trunc);
  if (!finite_f32(d_solid)) return REGNET_ERR_UNSUPPORTED;
  LatticeCall call{VoxelGrid{(int)nx, (int)ny, (int)nz, 0.0f, 0.0f, 0.0f, voxel_f}, Lattice{}, h};
  const GraspBox box{x_lo, x_hi, half_thickness, half_width, half_space, back_x};
  const int status = lattice_call_tail(&call, box, standoff, x_extent, B, origin3, volume && L && counts && values);
  if (status != REGNET_OK || B == 0) return status;
  const Planes planes = planes_of(const_cast<void*>(volume), nx * ny * nz);
  const VolumeView vol{planes.D, planes.W, call.grid, d_solid, (int)min_weight};
  hipLaunchKernelGGL(approach_volume_kernel, dim3((unsigned)B), dim3(AV_T), 0, as_stream(stream), vol, L, box, x_hi_per_grasp,
                     standoff, call.lat, counts, values);
  REGNET_LAUNCH_CHECK();
  return REGNET_OK;
}
