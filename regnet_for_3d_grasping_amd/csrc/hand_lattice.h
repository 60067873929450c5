// hand_lattice.h -- the lattice of samples of the swept hand and its lookup in a voxel grid, shared by every kernel that holds the
// hand against the TSDF volume (approach_volume.hip, view_gain.hip's interest kernel: voxel_class) or against its distance field
// (edt.hip's margin kernel, retreat.hip, hand_path.hip: field_lookup; hand_adjust.hip interpolates, sdf_sample.h): the lattice's
// counts and an entry point's checks on the host, the tile walk of a workgroup of 256 threads, and the sample's nearest voxel.
// include/regnet_hip.h ("approach analysis against the TSDF volume": lattice, sets, lookup) is the contract of them all.  The
// translation unit must be built with -ffp-contract=off (hand_box.h).
#pragma once
#include "hand_box.h"
#include "tsdf_volume.h"

#include <math.h>

constexpr int HL_T = 256;            // threads of a workgroup that walks the lattice
constexpr int HL_W = HL_T / 64;
constexpr int HL_TILE = 8;

struct Lattice {
  int nx, ny, nz;   // samples per axis
  float xs, h;      // x_lo - S (one float32 subtraction, made by the host function) and the step
};

struct VoxelGrid {  // where the voxels are: dims, the corner of voxel (0, 0, 0) and the edge
  int nx, ny, nz;
  float ox, oy, oz, voxel;
};

// The nearest voxel of the point (wx, wy, wz) of the grid's frame -> whether it is inside (a NaN is not), and then its linear
// index.  (Every dim <= 2^24: (float)n is exact and the test compares exact floats.)
__device__ __forceinline__ bool grid_voxel(const VoxelGrid& grid, float wx, float wy, float wz, int64_t& v) {
  const float fnx = (float)grid.nx, fny = (float)grid.ny, fnz = (float)grid.nz;
  const float cx = floorf(__fdiv_rn(wx - grid.ox, grid.voxel));
  const float cy = floorf(__fdiv_rn(wy - grid.oy, grid.voxel));
  const float cz = floorf(__fdiv_rn(wz - grid.oz, grid.voxel));
  const bool inside = cx >= 0.0f && cx < fnx && cy >= 0.0f && cy < fny && cz >= 0.0f && cz < fnz;   // (a NaN fails)
  if (inside) v = voxel_index<int64_t>((int)cx, (int)cy, (int)cz, grid.nx, grid.ny);
  return inside;
}

// The volume as a lookup reads it, and THE class of a looked-up voxel (include/regnet_hip.h "class"), which approach_volume.hip
// and view_gain.hip share: one W is loaded, and D only when W >= min_weight.
struct VolumeView {
  const float* D;
  const int32_t* W;
  VoxelGrid grid;
  float d_solid;
  int min_weight;
};

enum VoxelClass { VC_OUTSIDE = 0, VC_UNKNOWN = 1, VC_SOLID = 2, VC_FREE = 3 };

__device__ __forceinline__ VoxelClass voxel_class(const VolumeView& vol, bool inside, int64_t v) {
  if (!inside) return VC_OUTSIDE;
  if (vol.W[v] < vol.min_weight) return VC_UNKNOWN;
  const float d = vol.D[v];
  if (d != d) return VC_UNKNOWN;                     // a NaN distance
  return d < vol.d_solid ? VC_SOLID : VC_FREE;
}

// THE value of a looked-up voxel of a distance field (include/regnet_hip.h "distance field", the OUTSIDE rule): the field's word
// of the nearest voxel; a point outside the grid has no value when outside = 0 (the sample is skipped) and else lies in an
// obstacle: 0, or -1 of a SIGNED field (an obstacle of unknown depth; 0 is not a value of a signed field).
struct FieldLookup {
  bool inside, has_value;
};

template <bool SIGNED>
__device__ __forceinline__ FieldLookup field_lookup(const int32_t* __restrict__ field, const VoxelGrid& grid, int outside, float wx,
                                                    float wy, float wz, int& value) {
  int64_t v;
  const bool inside = grid_voxel(grid, wx, wy, wz, v);
  value = inside ? field[v] : (SIGNED ? -1 : 0);
  return FieldLookup{inside, inside || outside != 0};
}

// The walk of one workgroup of HL_T threads over the lattice: a wave takes 8 x 8 tiles of the x-y plane, tile t = wave, wave + 4,
// ..., lane l at (l & 7, l >> 3) of the tile, and walks the n_z layers.  visit(x, y, z, sets) is called for every sample of
// this thread, with hand_box.h's sets for the grasp's own x_hi.  lattice_walk_at also hands over the sample's place (i, j, k) in
// the lattice; lattice_point gives the coordinates of a place again, with the walk's own arithmetic.
__device__ __forceinline__ void lattice_point(const Lattice& lat, const GraspBox& box, int i, int j, int k, float& x, float& y,
                                              float& z) {
  x = lat.xs + (((float)i + 0.5f) * lat.h);
  y = (((float)j + 0.5f) * lat.h) - box.half_width;
  z = (((float)k + 0.5f) * lat.h) - box.half_thickness;
}

template <typename Visit>
__device__ __forceinline__ void lattice_walk_at(const Lattice& lat, const GraspBox& box, float x_hi, Visit visit) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int tiles_x = (lat.nx + HL_TILE - 1) / HL_TILE, tiles_y = (lat.ny + HL_TILE - 1) / HL_TILE;
  const int tiles = tiles_x * tiles_y;               // (at most 2^22 samples in all: no overflow)
  for (int t = wave; t < tiles; t += HL_W) {
    const int ty = t / tiles_x, tx = t - ty * tiles_x;
    const int i = tx * HL_TILE + (lane & (HL_TILE - 1)), j = ty * HL_TILE + (lane >> 3);
    if (i >= lat.nx || j >= lat.ny) continue;
    for (int k = 0; k < lat.nz; ++k) {
      float x, y, z;
      lattice_point(lat, box, i, j, k, x, y, z);
      visit(i, j, k, x, y, z, hand_sets(box, x_hi, lat.xs, x, y, z));
    }
  }
}

// (Kept beside lattice_walk_at, whose expressions it shares, out of caution: as a wrapper over it no check failed, but
// approach_volume_kernel and view_interest_kernel came out as other code, and as it stands they are unchanged;
// profiles/hand_field_refactor.txt.)
template <typename Visit>
__device__ __forceinline__ void lattice_walk(const Lattice& lat, const GraspBox& box, float x_hi, Visit visit) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int tiles_x = (lat.nx + HL_TILE - 1) / HL_TILE, tiles_y = (lat.ny + HL_TILE - 1) / HL_TILE;
  const int tiles = tiles_x * tiles_y;               // (at most 2^22 samples in all: no overflow)
  for (int t = wave; t < tiles; t += HL_W) {
    const int ty = t / tiles_x, tx = t - ty * tiles_x;
    const int i = tx * HL_TILE + (lane & (HL_TILE - 1)), j = ty * HL_TILE + (lane >> 3);
    if (i >= lat.nx || j >= lat.ny) continue;
    const float x = lat.xs + (((float)i + 0.5f) * lat.h);
    const float y = (((float)j + 0.5f) * lat.h) - box.half_width;
    for (int k = 0; k < lat.nz; ++k) {
      const float z = (((float)k + 0.5f) * lat.h) - box.half_thickness;
      visit(x, y, z, hand_sets(box, x_hi, lat.xs, x, y, z));
    }
  }
}

// ---- the host's half: the checks and counts of an entry point that takes a lattice -----------------------------------------
static inline bool positive_f32(double v, float* out) {   // finite and positive, in float32 too
  const float f = (float)v;
  *out = f;
  return v > 0.0 && f > 0.0f && f != __builtin_inff() && f == f;
}
static inline bool finite_f32(float f) { return f == f && f != __builtin_inff() && f != -__builtin_inff(); }

// max(1, ceil(extent / h)) in float64; false when it cannot be a lattice count (not finite, or beyond the sample limit)
static inline bool lattice_count(double extent, double h, int* n) {
  const double c = ceil(extent / h);
  if (!(c <= (double)(1 << 22)) || c == -__builtin_inf()) return false;   // (a NaN fails the first test)
  *n = c < 1.0 ? 1 : (int)c;
  return true;
}

// The lattice of a call (include/regnet_hip.h "lattice") -> false when a count is not finite or there are more than 2^22 samples.
static inline bool lattice_of(float x_lo, float standoff, float half_thickness, float half_width, float x_extent, float h,
                              Lattice* lat) {
  const float xs = x_lo - standoff;
  int n_x, n_y, n_z;
  if (!lattice_count((double)x_extent - (double)xs, (double)h, &n_x) ||
      !lattice_count((double)half_width + (double)half_width, (double)h, &n_y) ||
      !lattice_count((double)half_thickness + (double)half_thickness, (double)h, &n_z))
    return false;
  if ((int64_t)n_x * n_y * n_z > ((int64_t)1 << 22)) return false;
  *lat = Lattice{n_x, n_y, n_z, xs, h};
  return true;
}

// The dims of a distance field (edt.hip builds it; its margin kernel and retreat.hip read it): REGNET_OK, or the status of the
// first rule they break.
constexpr int FIELD_MAX_DIM = 1024;
static inline int field_dims(int64_t nx, int64_t ny, int64_t nz) {
  if (nx < 1 || ny < 1 || nz < 1) return REGNET_ERR_SHAPE;
  if (nx > FIELD_MAX_DIM || ny > FIELD_MAX_DIM || nz > FIELD_MAX_DIM || nx * ny * nz > ((int64_t)1 << 28)) return REGNET_ERR_UNSUPPORTED;
  return REGNET_OK;
}

// The checks of an entry point that holds the lattice against a grid, in the header's order, around the caller's own limit
// checks: field_call_checks (the entry points that read a distance field) opens, lattice_call_tail (those and the volume's) closes.
struct LatticeCall {
  VoxelGrid grid;   // dims and edge by the opening checks (or the caller), the corner by the tail
  Lattice lat;
  float h;
};

// B, outside, the field's dims, B < 2^31, voxel and step -> REGNET_OK, or the status of the first rule they break
static inline int field_call_checks(int64_t nx, int64_t ny, int64_t nz, double voxel, int outside, int64_t B, double step,
                                    LatticeCall* call) {
  if (B < 0 || outside < 0 || outside > 1) return REGNET_ERR_SHAPE;
  const int dims = field_dims(nx, ny, nz);
  if (dims != REGNET_OK) return dims;
  if (B >= (int64_t)1 << 31) return REGNET_ERR_UNSUPPORTED;
  float voxel_f;
  if (!positive_f32(voxel, &voxel_f) || !positive_f32(step, &call->h)) return REGNET_ERR_UNSUPPORTED;
  call->grid = VoxelGrid{(int)nx, (int)ny, (int)nz, 0.0f, 0.0f, 0.0f, voxel_f};
  return REGNET_OK;
}

// The standoff, the lattice, B == 0 (REGNET_OK: the caller returns without a launch) and the pointers; then the grid's corner.
static inline int lattice_call_tail(LatticeCall* call, const GraspBox& box, float standoff, float x_extent, int64_t B,
                                    const float* origin3, bool pointers) {
  if (!(standoff >= 0.0f) || standoff == __builtin_inff()) return REGNET_ERR_UNSUPPORTED;   // negative, NaN or infinite
  if (!lattice_of(box.x_lo, standoff, box.half_thickness, box.half_width, x_extent, call->h, &call->lat)) return REGNET_ERR_UNSUPPORTED;
  if (B == 0) return REGNET_OK;
  if (!origin3 || !pointers) return REGNET_ERR_NULL;
  call->grid.ox = origin3[0]; call->grid.oy = origin3[1]; call->grid.oz = origin3[2];
  return REGNET_OK;
}
