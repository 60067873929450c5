// edt.hip -- the exact Euclidean distance field of the TSDF volume on the device (gfx950), and what reads it: a point query and
// the per-grasp margin of the swept hand (include/regnet_hip.h "distance field").
//
// The transform is separable: with f0 = 0 on an obstacle voxel and NONE = 2^30 elsewhere, three line passes
//   g(i) = min_j f(j) + (i - j)^2
// along x, then y, then z leave the squared distance to the nearest obstacle, in voxel units, an integer.  A pass's 1D problem
// is solved by a search OUTWARD from i -- j = i - d, i + d for d = 1, 2, ... -- that stops once d^2 > best: f >= 0, so nothing
// further out can win or tie.  It is short wherever an obstacle is near, and a whole line where there is none.  Ties go to the
// smaller j: a left candidate takes `<=`, a right one `<` (every left candidate is smaller than all visited before it, every
// right one larger), so the obstacle recorded in `nearest` is the one of the smallest linear index (DESIGN.md par. 5).
//
// x pass: one wave per line, four lines per workgroup; the wave classifies its line straight from D / W into LDS (the rule of
// approach_volume.hip) and searches there; a line without an obstacle is stored without a search.  y and z pass: a workgroup
// stages a tile of T lines x n words in LDS (T consecutive ix on the lanes: the global loads and stores run along x), T the
// largest of 64, 32, 16, 8 that keeps the tile at or under 64 KiB; in LDS word j T + t the lanes of a wave read consecutive
// words at every step of the search: no bank conflict.  A workgroup owns its lines, so the passes run in place.  Integer work
// only: no atomics, no sort, no workgroup waits for another, and two runs give the same bytes.
//
// The SIGNED, CAPPED field (regnet_tsdf_sdf) is the same three passes run twice: once with the obstacles as seeds into `field`,
// once over the COMPLEMENT (the non-obstacle voxels as seeds) into the workspace, whose z pass folds the sign in -- a voxel whose
// positive value is 0 is an obstacle and takes minus its distance to free space; the tile, its bank argument and the tie rule are
// unchanged.  A cap of c voxels ends every search at d > c and turns an intermediate above c^2 into NONE: a voxel whose true
// squared distance is <= c^2 has every partial sum of its three terms <= c^2, so nothing it needs is lost; only the last pass
// writes c^2 into the words still above it.  The signed query interpolates the signed metres trilinearly, in a pinned order
// (sdf_sample.h, which the push-out of hand_adjust.hip shares).
#include "sdf_sample.h"

namespace {

constexpr int EDT_NONE = REGNET_EDT_NONE;
constexpr int EDT_T = 256;
constexpr int EDT_W = EDT_T / 64;
constexpr int EDT_MAX_DIM = FIELD_MAX_DIM;
constexpr int EDT_TILE_BYTES = 64 * 1024;

// min_j f[j stride] + (i - j)^2 over the n words of a line, and the smallest j that attains it (-1: none, best == NONE)
// `lim`: the search ends before d == lim (n: the whole line; cap + 1 under a cap)
__device__ __forceinline__ void line_search(const int* __restrict__ f, int stride, int n, int lim, int i, int& best, int& arg) {
  best = f[i * stride];
  arg = best < EDT_NONE ? i : -1;
  for (int d = 1; d < lim; ++d) {
    const int dd = d * d, jl = i - d, jr = i + d;
    if (dd > best || (jl < 0 && jr >= n)) break;
    if (jl >= 0) {
      const int c = f[jl * stride] + dd;             // (f <= 2^30, dd < 2^20: no overflow; f == NONE gives c > NONE >= best)
      if (c <= best) { best = c; arg = jl; }
    }
    if (jr < n) {
      const int c = f[jr * stride] + dd;
      if (c < best) { best = c; arg = jr; }
    }
  }
}

__global__ __launch_bounds__(EDT_T) void edt_x_kernel(const float* __restrict__ D, const int32_t* __restrict__ W, int nx, int lines,
                                                      int min_weight, float d_solid, int mode, int complement, int lim, int cap2,
                                                      int32_t* __restrict__ dist2, int32_t* __restrict__ nearest) {
  __shared__ int f[EDT_W][EDT_MAX_DIM];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int line = blockIdx.x * EDT_W + wave;
  const bool live = line < lines;
  const int base = line * nx;                        // (< 2^28 where live)
  bool mine = false;
  if (live) {
    for (int i = lane; i < nx; i += 64) {
      bool solid = false, unknown = true;
      if (W[base + i] >= min_weight) {
        const float d = D[base + i];
        unknown = d != d;                            // a NaN distance: UNKNOWN
        solid = d < d_solid;
      }
      const bool obstacle = solid || (mode != 0 && unknown);
      const bool seed = obstacle != (complement != 0);   // (the complement's seeds are the non-obstacle voxels)
      f[wave][i] = seed ? 0 : EDT_NONE;
      mine = mine || seed;
    }
  }
  const bool any = __ballot(mine) != 0ull;
  __syncthreads();
  if (!live) return;
  for (int i = lane; i < nx; i += 64) {
    int best = EDT_NONE, arg = -1;
    if (any) line_search(f[wave], 1, nx, lim, i, best, arg);
    if (best > cap2) { best = EDT_NONE; arg = -1; }  // (beyond the cap: as if there were none; uncapped cap2 == NONE: never)
    dist2[base + i] = best;
    if (nearest) nearest[base + i] = arg >= 0 ? base + arg : -1;
  }
}

struct LinePass {
  int nx, n;                    // voxels along x, and along the pass's axis
  int line_stride, outer_stride;   // words from one voxel of a line to the next, and from one tile row to the next
  int tiles_x, log_t;
  int outside, ny, nz;          // outside != 0 (the z pass only): fold the six faces in; then outer = iy and the line runs along z
  int lim, cap2, over;          // the search ends before d == lim; a result above cap2 becomes `over` (NONE, or cap2 in the last pass)
};

// `field` (the complement's z pass only): the plane of the positive side; a word that is 0 there is an obstacle and takes minus
// this pass's result (and `field_nearest` its way out), every other word is left alone and dist2 / nearest are not written.
__global__ __launch_bounds__(EDT_T) void edt_line_kernel(LinePass p, int32_t* __restrict__ dist2, int32_t* __restrict__ nearest,
                                                         int32_t* __restrict__ field, int32_t* __restrict__ field_nearest) {
  extern __shared__ int edt_lds[];
  const int T = 1 << p.log_t, total = p.n << p.log_t;
  int* f = edt_lds;
  int* from = edt_lds + total;                       // the nearest plane of the tile (only with `nearest`)
  const int outer = blockIdx.x / p.tiles_x, x0 = (blockIdx.x - outer * p.tiles_x) << p.log_t;
  const int base = outer * p.outer_stride + x0;
  const int width = min(T, p.nx - x0);
  for (int e = threadIdx.x; e < total; e += EDT_T) {
    const int t = e & (T - 1), j = e >> p.log_t;
    if (t >= width) continue;
    const int l = base + j * p.line_stride + t;
    f[e] = dist2[l];
    if (nearest) from[e] = nearest[l];
  }
  __syncthreads();
  for (int e = threadIdx.x; e < total; e += EDT_T) {
    const int t = e & (T - 1), i = e >> p.log_t;
    if (t >= width) continue;
    int best, arg;
    line_search(f + t, T, p.n, p.lim, i, best, arg);
    int near = (nearest && arg >= 0) ? from[(arg << p.log_t) + t] : -1;
    if (p.outside) {
      const int ix = x0 + t, iy = outer, iz = i;
      const int m = min(min(min(ix + 1, p.nx - ix), min(iy + 1, p.ny - iy)), min(iz + 1, p.nz - iz));
      if (m * m < best) { best = m * m; near = -1; }   // (strictly nearer: an interior obstacle wins a tie)
    }
    if (best > p.cap2) { best = p.over; near = -1; }
    const int l = base + i * p.line_stride + t;
    if (field) {
      if (field[l] == 0) {
        field[l] = -best;
        if (field_nearest) field_nearest[l] = near;
      }
      continue;
    }
    dist2[l] = best;
    if (nearest) nearest[l] = near;
  }
}

// (float)d2 is exact (d2 <= 3 * 1023^2 < 2^24), sqrtf is correctly rounded, one multiplication
__device__ __forceinline__ float edt_metres(int d2, float voxel) {
  return d2 >= EDT_NONE ? __builtin_inff() : (sqrtf((float)d2) * voxel) + 0.0f;
}

__device__ __forceinline__ float canonical_nan(float v) { return v != v ? __builtin_nanf("") : v; }

struct Rows12 {
  float r[3][4];
};

__global__ __launch_bounds__(EDT_T) void edt_query_signed_kernel(const int32_t* __restrict__ field,
                                                                 const int32_t* __restrict__ nearest, VoxelGrid grid,
                                                                 const float* __restrict__ points, int64_t stride_row,
                                                                 int64_t stride_col, int64_t M, Rows12 T, int interpolate,
                                                                 float* __restrict__ distance, float* __restrict__ gradient,
                                                                 float* __restrict__ nearest_xyz) {
  const int64_t m = (int64_t)blockIdx.x * EDT_T + threadIdx.x;
  if (m >= M) return;
  const float* q = points + m * stride_row;
  const float px = q[0], py = q[stride_col], pz = q[2 * stride_col];
  const float wx = affine3(T.r[0], px, py, pz), wy = affine3(T.r[1], px, py, pz), wz = affine3(T.r[2], px, py, pz);
  const float nan = __builtin_nanf("");
  float dist = nan, gx = nan, gy = nan, gz = nan, cx = nan, cy = nan, cz = nan;
  int64_t v;
  if (grid_voxel(grid, wx, wy, wz, v)) {
    const float vox = grid.voxel;
    if (interpolate) {
      dist = sdf_sample(field, grid, wx, wy, wz, gradient != nullptr, gx, gy, gz);
    } else {
      dist = sdf_metres(field[v], vox);
    }
    const int near = nearest ? nearest[v] : -1;
    if (near >= 0) {
      const int ix = near % grid.nx, r = near / grid.nx;
      cx = centre(grid.ox, ix, vox);
      cy = centre(grid.oy, r % grid.ny, vox);
      cz = centre(grid.oz, r / grid.ny, vox);
    }
  }
  distance[m] = canonical_nan(dist);
  if (gradient) {
    gradient[3 * m] = canonical_nan(gx); gradient[3 * m + 1] = canonical_nan(gy); gradient[3 * m + 2] = canonical_nan(gz);
  }
  if (nearest_xyz) {
    nearest_xyz[3 * m] = cx; nearest_xyz[3 * m + 1] = cy; nearest_xyz[3 * m + 2] = cz;
  }
}

__global__ __launch_bounds__(EDT_T) void edt_metres_signed_kernel(const int32_t* __restrict__ field, int64_t n, float voxel,
                                                                  float* __restrict__ out) {
  const int64_t l = (int64_t)blockIdx.x * EDT_T + threadIdx.x;
  if (l < n) out[l] = sdf_metres(field[l], voxel);
}

__global__ __launch_bounds__(EDT_T) void edt_query_kernel(const int32_t* __restrict__ dist2, const int32_t* __restrict__ nearest,
                                                          VoxelGrid grid, const float* __restrict__ points, int64_t stride_row,
                                                          int64_t stride_col, int64_t M, Rows12 T, float* __restrict__ distance,
                                                          float* __restrict__ nearest_xyz) {
  const int64_t m = (int64_t)blockIdx.x * EDT_T + threadIdx.x;
  if (m >= M) return;
  const float* q = points + m * stride_row;
  const float px = q[0], py = q[stride_col], pz = q[2 * stride_col];
  const float wx = affine3(T.r[0], px, py, pz), wy = affine3(T.r[1], px, py, pz), wz = affine3(T.r[2], px, py, pz);
  const float nan = __builtin_nanf("");
  float dist = nan, cx = nan, cy = nan, cz = nan;
  int64_t v;
  if (grid_voxel(grid, wx, wy, wz, v)) {
    dist = edt_metres(dist2[v], grid.voxel);
    const int near = nearest ? nearest[v] : -1;
    if (near >= 0) {
      const int ix = near % grid.nx, r = near / grid.nx;
      cx = centre(grid.ox, ix, grid.voxel);
      cy = centre(grid.oy, r % grid.ny, grid.voxel);
      cz = centre(grid.oz, r / grid.ny, grid.voxel);
    }
  }
  distance[m] = dist;
  if (nearest_xyz) {
    nearest_xyz[3 * m] = cx; nearest_xyz[3 * m + 1] = cy; nearest_xyz[3 * m + 2] = cz;
  }
}

__global__ __launch_bounds__(EDT_T) void edt_metres_kernel(const int32_t* __restrict__ dist2, int64_t n, float voxel,
                                                           float* __restrict__ out) {
  const int64_t l = (int64_t)blockIdx.x * EDT_T + threadIdx.x;
  if (l < n) out[l] = edt_metres(dist2[l], voxel);
}

// SIGNED: the plane is a signed field -- an OUTSIDE sample under outside = 1 contributes -1 (an obstacle of unknown depth; 0 is
// not a value of a signed field) and counts gains the hand and the swept samples with a negative value
template <bool SIGNED>
__global__ __launch_bounds__(HL_T) void edt_margin_kernel(const int32_t* __restrict__ dist2, VoxelGrid grid, int outside,
                                                          const float* __restrict__ L, GraspBox box,
                                                          const float* __restrict__ x_hi_per_grasp, Lattice lat,
                                                          int32_t* __restrict__ margins, int32_t* __restrict__ counts) {
  constexpr int EM_NI = SIGNED ? 6 : 4;
  __shared__ int red_i[EM_NI][HL_W];
  __shared__ int red_m[2][HL_W];
  const GraspRows g = grasp_rows(L, blockIdx.x, 12);
  const float x_hi = x_hi_per_grasp ? x_hi_per_grasp[blockIdx.x] : box.x_hi;
  int hand_n = 0, hand_out = 0, sweep_n = 0, sweep_out = 0, hand_neg = 0, sweep_neg = 0;
  int hand_min = EDT_NONE, sweep_min = EDT_NONE;
  lattice_walk(lat, box, x_hi, [&](float x, float y, float z, const HandSets& in) {
    const bool hand = in.back || in.finger;
    if (!(hand || in.blocker)) return;               // not in the swept set: no lookup
    float wx, wy, wz;
    grasp_apply(g, x, y, z, wx, wy, wz);
    int d2;
    const FieldLookup at = field_lookup<SIGNED>(dist2, grid, outside, wx, wy, wz, d2);
    sweep_n += 1;
    hand_n += (int)hand;
    if (!at.inside) {
      sweep_out += 1;
      hand_out += (int)hand;
    }
    if (!at.has_value) return;                       // an OUTSIDE sample under outside = 0: counted and skipped
    sweep_min = min(sweep_min, d2);
    if (hand) hand_min = min(hand_min, d2);
    if (SIGNED && d2 < 0) {
      sweep_neg += 1;
      hand_neg += (int)hand;
    }
  });
  int ri[6] = {hand_n, hand_out, sweep_n, sweep_out, hand_neg, sweep_neg};
#pragma unroll
  for (int q = 0; q < EM_NI; ++q) ri[q] = wave_sum(ri[q]);
  hand_min = wave_min(hand_min); sweep_min = wave_min(sweep_min);
#pragma unroll
  for (int q = 0; q < EM_NI; ++q) block_put(ri[q], red_i[q]);
  block_put(hand_min, red_m[0]); block_put(sweep_min, red_m[1]);
  __syncthreads();
  if (threadIdx.x == 0) {
    int32_t* c = counts + (int64_t)blockIdx.x * EM_NI;
#pragma unroll
    for (int q = 0; q < EM_NI; ++q) c[q] = block_sum<HL_W>(red_i[q]);
    margins[(int64_t)blockIdx.x * 2] = block_min<HL_W>(red_m[0]);
    margins[(int64_t)blockIdx.x * 2 + 1] = block_min<HL_W>(red_m[1]);
  }
}

// log2 of the lines per tile of a pass along an axis of n voxels: the largest of 64, 32, 16, 8 within 64 KiB
int tile_log(int64_t n, int words) {
  int log_t = 6;
  while (log_t > 3 && ((n * words * 4) << log_t) > EDT_TILE_BYTES) --log_t;
  return log_t;
}

}  // namespace

extern "C" int regnet_edt_tile(int64_t n, int with_nearest) {
  if (n < 1 || n > EDT_MAX_DIM) return REGNET_ERR_UNSUPPORTED;
  return 1 << tile_log(n, with_nearest ? 2 : 1);
}

namespace {

// the checks of a field call, all before any launch, in the header's order (cap: 0 for an entry without one)
int field_checks(const void* volume, int64_t nx, int64_t ny, int64_t nz, double trunc, int64_t min_weight, double margin, int mode,
                 int outside, int64_t cap, const int32_t* dist2) {
  if (min_weight < 1 || mode < 0 || mode > 1 || outside < 0 || outside > 1 || cap < 0) return REGNET_ERR_SHAPE;
  const int dims = field_dims(nx, ny, nz);
  if (dims != REGNET_OK) return dims;
  if (min_weight >= (int64_t)1 << 31 || cap > EDT_MAX_DIM - 1) return REGNET_ERR_UNSUPPORTED;
  const float trunc_f = (float)trunc, margin_f = (float)margin, d_solid = (float)(margin / trunc);
  if (!finite_f32(trunc_f) || !finite_f32(margin_f) || !finite_f32(d_solid)) return REGNET_ERR_UNSUPPORTED;
  if (!volume || !dist2) return REGNET_ERR_NULL;
  return REGNET_OK;
}

// One line pass (0, 1, 2: x, y, z) of a transform into dist2 / nearest, the arguments already checked.  cap: 0 or 1..1023;
// complement: the seeds are the NON-obstacle voxels; last: this transform's z pass writes cap^2 into the words beyond the cap;
// field / field_nearest (the complement's z pass): fold the result into the positive side's planes instead of storing it.
void launch_pass(const void* volume, int64_t nx, int64_t ny, int64_t nz, double trunc, int64_t min_weight, double margin, int mode,
                 int outside, int pass, int cap, int complement, int32_t* dist2, int32_t* nearest, int32_t* field,
                 int32_t* field_nearest, void* stream) {
  const int64_t n = nx * ny * nz;
  const int cap2 = cap ? cap * cap : EDT_NONE;
  if (pass == 0) {
    const float d_solid = (float)(margin / trunc);
    const Planes planes = planes_of(const_cast<void*>(volume), n);
    const int lines = (int)(ny * nz);
    const int lim = cap ? (int)(nx < cap + 1 ? nx : cap + 1) : (int)nx;
    hipLaunchKernelGGL(edt_x_kernel, dim3((unsigned)((lines + EDT_W - 1) / EDT_W)), dim3(EDT_T), 0, as_stream(stream), planes.D,
                       planes.W, (int)nx, lines, (int)min_weight, d_solid, mode, complement, lim, cap2, dist2, nearest);
  } else {
    const int words = nearest ? 2 : 1;
    const int64_t len = pass == 1 ? ny : nz, rows = pass == 1 ? nz : ny;
    const int log_t = tile_log(len, words);
    const int tiles_x = (int)((nx + (1 << log_t) - 1) >> log_t);
    const int lim = cap ? (int)(len < cap + 1 ? len : cap + 1) : (int)len;
    const LinePass p{(int)nx, (int)len, (int)(pass == 1 ? nx : nx * ny), (int)(pass == 1 ? nx * ny : nx), tiles_x, log_t,
                     pass == 2 ? outside : 0, (int)ny, (int)nz, lim, cap2, pass == 2 ? cap2 : EDT_NONE};
    const size_t lds = (size_t)((len * words * 4) << log_t);
    hipLaunchKernelGGL(edt_line_kernel, dim3((unsigned)(tiles_x * rows)), dim3(EDT_T), lds, as_stream(stream), p, dist2, nearest,
                       field, field_nearest);
  }
}

}  // namespace

extern "C" int regnet_tsdf_edt_pass(const void* volume, int64_t nx, int64_t ny, int64_t nz, double trunc, int64_t min_weight,
                                    double margin, int mode, int outside, int pass, int32_t* dist2, int32_t* nearest,
                                    void* stream) {
  if (pass < 0 || pass > 2) return REGNET_ERR_SHAPE;
  const int status = field_checks(volume, nx, ny, nz, trunc, min_weight, margin, mode, outside, 0, dist2);
  if (status != REGNET_OK) return status;
  launch_pass(volume, nx, ny, nz, trunc, min_weight, margin, mode, outside, pass, 0, 0, dist2, nearest, nullptr, nullptr, stream);
  REGNET_LAUNCH_CHECK();
  return REGNET_OK;
}

extern "C" int regnet_tsdf_edt(const void* volume, int64_t nx, int64_t ny, int64_t nz, double trunc, int64_t min_weight,
                               double margin, int mode, int outside, int32_t* dist2, int32_t* nearest, void* stream) {
  for (int pass = 0; pass < 3; ++pass) {             // (every check is made by the first call, before any launch)
    const int status = regnet_tsdf_edt_pass(volume, nx, ny, nz, trunc, min_weight, margin, mode, outside, pass, dist2, nearest,
                                            stream);
    if (status != REGNET_OK) return status;
  }
  return REGNET_OK;
}

extern "C" int64_t regnet_tsdf_sdf_workspace_bytes(int64_t nx, int64_t ny, int64_t nz, int sign, int with_nearest) {
  if (sign != 1 || field_dims(nx, ny, nz) != REGNET_OK) return 0;
  return nx * ny * nz * 4 * (with_nearest ? 2 : 1);  // the complement's dist2 plane, then its nearest plane
}

extern "C" int regnet_tsdf_sdf(const void* volume, int64_t nx, int64_t ny, int64_t nz, double trunc, int64_t min_weight,
                               double margin, int mode, int outside, int sign, int64_t cap, int32_t* field, int32_t* nearest,
                               void* work, void* stream) {
  if (sign < 0 || sign > 1) return REGNET_ERR_SHAPE;
  const int status = field_checks(volume, nx, ny, nz, trunc, min_weight, margin, mode, outside, cap, field);
  if (status != REGNET_OK) return status;
  if (sign && !work) return REGNET_ERR_NULL;
  for (int pass = 0; pass < 3; ++pass) {
    launch_pass(volume, nx, ny, nz, trunc, min_weight, margin, mode, outside, pass, (int)cap, 0, field, nearest, nullptr, nullptr,
                stream);
    REGNET_LAUNCH_CHECK();
  }
  if (sign) {
    int32_t* neg = static_cast<int32_t*>(work);
    int32_t* neg_nearest = nearest ? neg + nx * ny * nz : nullptr;
    for (int pass = 0; pass < 3; ++pass) {           // (the outside is never free space: it does not enter the negative side)
      launch_pass(volume, nx, ny, nz, trunc, min_weight, margin, mode, 0, pass, (int)cap, 1, neg, neg_nearest,
                  pass == 2 ? field : nullptr, pass == 2 ? nearest : nullptr, stream);
      REGNET_LAUNCH_CHECK();
    }
  }
  return REGNET_OK;
}

extern "C" int regnet_edt_query_f32(const int32_t* dist2, const int32_t* nearest, int64_t nx, int64_t ny, int64_t nz,
                                    const float* origin3, double voxel, const float* points, int64_t stride_row,
                                    int64_t stride_col, int64_t M, const float* T12, float* distance, float* nearest_xyz,
                                    void* stream) {
  if (M < 0) return REGNET_ERR_SHAPE;
  const int dims = field_dims(nx, ny, nz);
  if (dims != REGNET_OK) return dims;
  float voxel_f;
  if (M >= (int64_t)1 << 31 || !positive_f32(voxel, &voxel_f)) return REGNET_ERR_UNSUPPORTED;
  if (M == 0) return REGNET_OK;
  if (!dist2 || !origin3 || !points || !T12 || !distance) return REGNET_ERR_NULL;
  Rows12 T;
  for (int k = 0; k < 12; ++k) T.r[k >> 2][k & 3] = T12[k];
  const VoxelGrid grid{(int)nx, (int)ny, (int)nz, origin3[0], origin3[1], origin3[2], voxel_f};
  hipLaunchKernelGGL(edt_query_kernel, dim3((unsigned)((M + EDT_T - 1) / EDT_T)), dim3(EDT_T), 0, as_stream(stream), dist2, nearest,
                     grid, points, stride_row, stride_col, M, T, distance, nearest_xyz);
  REGNET_LAUNCH_CHECK();
  return REGNET_OK;
}

extern "C" int regnet_edt_query_signed_f32(const int32_t* field, const int32_t* nearest, int64_t nx, int64_t ny, int64_t nz,
                                           const float* origin3, double voxel, const float* points, int64_t stride_row,
                                           int64_t stride_col, int64_t M, const float* T12, int interpolate, float* distance,
                                           float* gradient, float* nearest_xyz, void* stream) {
  if (M < 0 || interpolate < 0 || interpolate > 1) return REGNET_ERR_SHAPE;
  const int dims = field_dims(nx, ny, nz);
  if (dims != REGNET_OK) return dims;
  float voxel_f;
  if (M >= (int64_t)1 << 31 || !positive_f32(voxel, &voxel_f)) return REGNET_ERR_UNSUPPORTED;
  if (M == 0) return REGNET_OK;
  if (!field || !origin3 || !points || !T12 || !distance) return REGNET_ERR_NULL;
  Rows12 T;
  for (int k = 0; k < 12; ++k) T.r[k >> 2][k & 3] = T12[k];
  const VoxelGrid grid{(int)nx, (int)ny, (int)nz, origin3[0], origin3[1], origin3[2], voxel_f};
  hipLaunchKernelGGL(edt_query_signed_kernel, dim3((unsigned)((M + EDT_T - 1) / EDT_T)), dim3(EDT_T), 0, as_stream(stream), field,
                     nearest, grid, points, stride_row, stride_col, M, T, interpolate, distance, gradient, nearest_xyz);
  REGNET_LAUNCH_CHECK();
  return REGNET_OK;
}

extern "C" int regnet_edt_metres_f32(const int32_t* dist2, int64_t n, double voxel, float* out, void* stream) {
  if (n < 0) return REGNET_ERR_SHAPE;
  float voxel_f;
  if (n > ((int64_t)1 << 28) || !positive_f32(voxel, &voxel_f)) return REGNET_ERR_UNSUPPORTED;
  if (n == 0) return REGNET_OK;
  if (!dist2 || !out) return REGNET_ERR_NULL;
  hipLaunchKernelGGL(edt_metres_kernel, dim3((unsigned)((n + EDT_T - 1) / EDT_T)), dim3(EDT_T), 0, as_stream(stream), dist2, n,
                     voxel_f, out);
  REGNET_LAUNCH_CHECK();
  return REGNET_OK;
}

extern "C" int regnet_edt_metres_signed_f32(const int32_t* field, int64_t n, double voxel, float* out, void* stream) {
  if (n < 0) return REGNET_ERR_SHAPE;
  float voxel_f;
  if (n > ((int64_t)1 << 28) || !positive_f32(voxel, &voxel_f)) return REGNET_ERR_UNSUPPORTED;
  if (n == 0) return REGNET_OK;
  if (!field || !out) return REGNET_ERR_NULL;
  hipLaunchKernelGGL(edt_metres_signed_kernel, dim3((unsigned)((n + EDT_T - 1) / EDT_T)), dim3(EDT_T), 0, as_stream(stream), field,
                     n, voxel_f, out);
  REGNET_LAUNCH_CHECK();
  return REGNET_OK;
}

namespace {

template <bool SIGNED>
int margin_volume(const int32_t* dist2, int64_t nx, int64_t ny, int64_t nz, const float* origin3, double voxel, int outside,
                  const float* L, int64_t B, float x_lo, float x_hi, const float* x_hi_per_grasp, float half_thickness,
                  float half_width, float half_space, float back_x, float standoff, double step, float x_extent, int32_t* margins,
                  int32_t* counts, void* stream) {
  LatticeCall call;
  int status = field_call_checks(nx, ny, nz, voxel, outside, B, step, &call);
  if (status != REGNET_OK) return status;
  const GraspBox box{x_lo, x_hi, half_thickness, half_width, half_space, back_x};
  status = lattice_call_tail(&call, box, standoff, x_extent, B, origin3, dist2 && L && margins && counts);
  if (status != REGNET_OK || B == 0) return status;
  hipLaunchKernelGGL(edt_margin_kernel<SIGNED>, dim3((unsigned)B), dim3(HL_T), 0, as_stream(stream), dist2, call.grid, outside, L,
                     box, x_hi_per_grasp, call.lat, margins, counts);
  REGNET_LAUNCH_CHECK();
  return REGNET_OK;
}

}  // namespace

extern "C" int regnet_grasp_margin_volume_f32(const int32_t* dist2, int64_t nx, int64_t ny, int64_t nz, const float* origin3,
                                              double voxel, int outside, const float* L, int64_t B, float x_lo, float x_hi,
                                              const float* x_hi_per_grasp, float half_thickness, float half_width,
                                              float half_space, float back_x, float standoff, double step, float x_extent,
                                              int32_t* margins, int32_t* counts, void* stream) {
  return margin_volume<false>(dist2, nx, ny, nz, origin3, voxel, outside, L, B, x_lo, x_hi, x_hi_per_grasp, half_thickness,
                              half_width, half_space, back_x, standoff, step, x_extent, margins, counts, stream);
}

extern "C" int regnet_grasp_margin_volume_signed_f32(const int32_t* field, int64_t nx, int64_t ny, int64_t nz, const float* origin3,
                                                     double voxel, int outside, const float* L, int64_t B, float x_lo, float x_hi,
                                                     const float* x_hi_per_grasp, float half_thickness, float half_width,
                                                     float half_space, float back_x, float standoff, double step, float x_extent,
                                                     int32_t* margins, int32_t* counts, void* stream) {
  return margin_volume<true>(field, nx, ny, nz, origin3, voxel, outside, L, B, x_lo, x_hi, x_hi_per_grasp, half_thickness,
                             half_width, half_space, back_x, standoff, step, x_extent, margins, counts, stream);
}
