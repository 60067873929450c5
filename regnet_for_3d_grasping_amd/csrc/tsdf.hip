// tsdf.hip -- depth views fused into a truncated signed distance volume and its surface extracted, on the device (gfx950).
//
// The contract is DESIGN.md par. 5 "TSDF volume" and include/regnet_hip.h.  Built with -ffp-contract=off: every product, sum,
// difference and division below is an individually rounded binary32 operation in the written order, so a numpy float32
// restatement (tests/tsdf_reference.py) gives the same bits.  One thread owns one voxel: no floating-point atomic, no sum whose
// order is open.
//
//   * tsdf_reset_kernel: D = 1, W = 0, C = 0.
//   * tsdf_clear_kernel: one workgroup zeroes the four counters of a call (a kernel and not a memset: a captured call stays one
//     chain of kernel nodes).
//   * tsdf_integrate_kernel: a 64 x 4 tile of voxels per 256-thread workgroup, ix on the lane, so a wave reads and writes 256
//     contiguous bytes of each of the five planes, over 16 z layers one after the other: the histogram collects in LDS and
//     costs four global atomics per workgroup (one per layer made 128 000 same-address atomics the whole time of the call at
//     320^3).  The depth image is gathered (it stays in cache); the volume is streamed once.  A layer none of whose voxels is
//     in view is left after the projection; a workgroup all of whose layers are leaves without touching the volume.
//   * tsdf_count_kernel / tsdf_emit_kernel: blocks of 256 consecutive linear voxel indices, three candidates per voxel.  The
//     count pass (16 blocks per workgroup, one after the other) leaves the kept candidates per block; the caller's exclusive
//     prefix sum gives every block its first row; the emit pass recomputes the predicate and ranks in key order (three ballots
//     per wave, the waves' totals through LDS).
//   * tsdf_tail_kernel: the sentinels beyond the K rows, and num.
//   * tsdf_raycast_kernel: a lane per pixel of a virtual pinhole camera marches its ray through the volume, which it only reads
//     (tests/tsdf_raycast_reference.py restates it).  A wave is an 8 x 8 pixel tile, so its 64 rays stay in neighbouring cells
//     and their eight corner loads fall on few cache lines.  Every ray starts and ends at the samples a float64 slab test
//     against the box of voxel centres leaves it (conservatively: the samples skipped are unknown by the sample rule, so the
//     clip changes no bit).  The histogram collects in LDS as integrate's does.
// The launches are ordered by the stream: no workgroup waits for another, no flags, no cooperative launch.
#include "ray_clip.h"
#include "tsdf_volume.h"

namespace {

constexpr long long TS_MAX_VOXELS = 1ll << 28;
constexpr long long TS_MAX_PIXELS = 1ll << 21;      // ingest.MAX_FRAME_POINTS
constexpr long long TS_MAX_POINTS = 1ll << 21;
constexpr int TS_TX = 64, TS_TY = 4;                // the integrate tile: a wave is 64 consecutive ix of one (iy, iz)
constexpr int TS_TZ = 16;                           // ... over so many z layers, one after the other: 16 times fewer global atomics
constexpr int TS_CB = 16;                           // blocks of 256 voxels per workgroup of the count pass, for the same reason
constexpr int TS_BLOCK = TS_TX * TS_TY;
constexpr int TS_WAVES = TS_BLOCK / 64;
constexpr unsigned TS_QNAN = 0x7FC00000u;

enum { TS_UPDATED = 0, TS_NOT_IN_VIEW = 1, TS_NO_DEPTH = 2, TS_BEHIND = 3, TS_CODES = 4 };

struct IntegrateArgs {
  int nx, ny, nz, tiles_x, tiles_y;
  int width, height, max_weight;
  float o[3], voxel, trunc, rtrunc;
  float fx, fy, cx, cy;
  float r[12];
};

__global__ __launch_bounds__(TS_BLOCK) void tsdf_reset_kernel(Planes p, long long n) {
  const long long l = (long long)blockIdx.x * TS_BLOCK + threadIdx.x;
  if (l >= n) return;
  p.D[l] = 1.0f;
  p.W[l] = 0;
  p.C[0][l] = 0.0f; p.C[1][l] = 0.0f; p.C[2][l] = 0.0f;
}

__global__ __launch_bounds__(64) void tsdf_clear_kernel(int32_t* __restrict__ counts) {
  if (threadIdx.x < TS_CODES) counts[threadIdx.x] = 0;
}

__global__ __launch_bounds__(TS_BLOCK) void tsdf_integrate_kernel(Planes p, const IntegrateArgs a, const float* __restrict__ xyz,
                                                                  const float* __restrict__ rgb, int32_t* __restrict__ counts) {
  __shared__ int s_hist[TS_CODES];
  const int tid = threadIdx.x;
  unsigned b = blockIdx.x;
  const int tx = (int)(b % (unsigned)a.tiles_x);
  b /= (unsigned)a.tiles_x;
  const int ty = (int)(b % (unsigned)a.tiles_y);
  const int z0 = (int)(b / (unsigned)a.tiles_y) * TS_TZ, z1 = min(z0 + TS_TZ, a.nz);
  const int ix = tx * TS_TX + (tid & 63), iy = ty * TS_TY + (tid >> 6);
  const bool active = ix < a.nx && iy < a.ny;
  const int tile_voxels = min(TS_TX, a.nx - tx * TS_TX) * min(TS_TY, a.ny - ty * TS_TY);
  if (tid < TS_CODES) s_hist[tid] = 0;
  __syncthreads();
  const float px = centre(a.o[0], ix, a.voxel), py = centre(a.o[1], iy, a.voxel);
  for (int iz = z0; iz < z1; ++iz) {
    int code = TS_NOT_IN_VIEW;
    int pixel = 0;
    float z = 0.0f;
    if (active) {
      const float pz = centre(a.o[2], iz, a.voxel);
      const float x = affine3(a.r, px, py, pz), y = affine3(a.r + 4, px, py, pz);
      z = affine3(a.r + 8, px, py, pz);
      if (__builtin_isfinite(z) && z > 0.0f) {
        const float u = (__fdiv_rn(x, z) * a.fx) + a.cx;
        const float v = (__fdiv_rn(y, z) * a.fy) + a.cy;
        const float fu = floorf(u + 0.5f), fv = floorf(v + 0.5f);
        if (fu >= 0.0f && fu < (float)a.width && fv >= 0.0f && fv < (float)a.height) {      // in float: a NaN fails
          code = TS_NO_DEPTH;
          pixel = (int)fv * a.width + (int)fu;
        }
      }
    }
    // the early exit: the same per-voxel test as below, so the result does not depend on it
    if (__syncthreads_or(code != TS_NOT_IN_VIEW) == 0) {
      if (tid == 0) atomicAdd(&s_hist[TS_NOT_IN_VIEW], tile_voxels);
      continue;
    }
    if (code == TS_NO_DEPTH) {
      const float zd = xyz[(long long)pixel * 3 + 2];
      if (__builtin_isfinite(zd)) {
        const float sdf = zd - z;
        code = TS_BEHIND;
        if (!(sdf < -a.trunc)) {
          code = TS_UPDATED;
          const float t = fminf(sdf * a.rtrunc, 1.0f);
          const long long l = voxel_index<long long>(ix, iy, iz, a.nx, a.ny);
          // every load before the first store: the five planes are one allocation, which the compiler must take to alias
          const int w = p.W[l];
          const float d = p.D[l];
          float c[3], colour[3];
#pragma unroll
          for (int k = 0; k < 3; ++k) {
            c[k] = p.C[k][l];
            colour[k] = rgb ? rgb[(long long)pixel * 3 + k] : 0.0f;
          }
          const float wf = (float)w, w1 = wf + 1.0f;
          p.D[l] = __fdiv_rn((d * wf) + t, w1);
#pragma unroll
          for (int k = 0; k < 3; ++k) p.C[k][l] = __fdiv_rn((c[k] * wf) + colour[k], w1);
          p.W[l] = min(w + 1, a.max_weight);
        }
      }
    }
#pragma unroll
    for (int c = 0; c < TS_CODES; ++c) {
      const int n = __popcll(__ballot(active && code == c));
      if (lane_id() == 0 && n != 0) atomicAdd(&s_hist[c], n);
    }
  }
  // one integer atomic per workgroup and code
  __syncthreads();
  if (tid < TS_CODES) {
    const int n = s_hist[tid];
    if (n != 0) atomicAdd(&counts[tid], n);
  }
}

__global__ __launch_bounds__(TS_BLOCK) void tsdf_count_kernel(const float* __restrict__ D, const int32_t* __restrict__ W,
                                                              const ExtractArgs a, int32_t* __restrict__ block_counts,
                                                              int32_t* __restrict__ num) {
  __shared__ int s_kept[TS_WAVES], s_seen[TS_WAVES];
  const int blocks = (a.n + TS_BLOCK - 1) / TS_BLOCK;
  const int first = (int)blockIdx.x * TS_CB, last = min(first + TS_CB, blocks);
  int seen_all = 0;                                   // (thread 0's)
  for (int block = first; block < last; ++block) {
    const int l = block * TS_BLOCK + (int)threadIdx.x;
    int bits = 0;
    bool observed = false;
    if (l < a.n) {
      int ix, iy, iz;
      tsdf_index(a, l, ix, iy, iz);
      bits = tsdf_kept(D, W, a, l, ix, iy, iz, observed);
    }
    const int kept = __popcll(__ballot(bits & 1)) + __popcll(__ballot(bits & 2)) + __popcll(__ballot(bits & 4));
    const int seen = __popcll(__ballot(observed));
    if (lane_id() == 0) { s_kept[threadIdx.x >> 6] = kept; s_seen[threadIdx.x >> 6] = seen; }
    __syncthreads();
    if (threadIdx.x == 0) {
      int k = 0;
#pragma unroll
      for (int w = 0; w < TS_WAVES; ++w) { k += s_kept[w]; seen_all += s_seen[w]; }
      block_counts[block] = k;
    }
    __syncthreads();
  }
  if (threadIdx.x == 0 && seen_all != 0) atomicAdd(&num[2], seen_all);      // one integer atomic per workgroup
}

// the central, or one-sided, difference of D along one axis at voxel l (index i of extent `extent`, `step` words to the neighbour)
__device__ __forceinline__ float tsdf_gradient(const float* __restrict__ D, const int32_t* __restrict__ W, int min_weight, int l,
                                               int i, int extent, int step) {
  const bool lo = i > 0 && W[l - step] >= min_weight;
  const bool hi = i + 1 < extent && W[l + step] >= min_weight;
  if (lo && hi) return D[l + step] - D[l - step];
  if (hi) return (D[l + step] - D[l]) * 2.0f;
  if (lo) return (D[l] - D[l - step]) * 2.0f;
  return 0.0f;
}

__global__ __launch_bounds__(TS_BLOCK) void tsdf_emit_kernel(const float* __restrict__ D, const int32_t* __restrict__ W,
                                                             const float* __restrict__ Cr, const float* __restrict__ Cg,
                                                             const float* __restrict__ Cb, const ExtractArgs a, float ox, float oy,
                                                             float oz, float voxel, const int32_t* __restrict__ block_base,
                                                             int max_points, float* __restrict__ xyz, float* __restrict__ rgb,
                                                             float* __restrict__ normal, int32_t* __restrict__ weight) {
  __shared__ int s_total[TS_WAVES];
  const int l = (int)(blockIdx.x * (unsigned)TS_BLOCK + threadIdx.x);
  int bits = 0, ix = 0, iy = 0, iz = 0;
  if (l < a.n) {
    bool observed;
    tsdf_index(a, l, ix, iy, iz);
    bits = tsdf_kept(D, W, a, l, ix, iy, iz, observed);
  }
  const uint64_t b0 = __ballot(bits & 1), b1 = __ballot(bits & 2), b2 = __ballot(bits & 4);
  const int wave = threadIdx.x >> 6;
  if (lane_id() == 0) s_total[wave] = __popcll(b0) + __popcll(b1) + __popcll(b2);
  __syncthreads();
  if (bits == 0) return;
  long long row = (long long)block_base[blockIdx.x] + mbcnt64(b0) + mbcnt64(b1) + mbcnt64(b2);
  for (int w = 0; w < wave; ++w) row += s_total[w];
  const int extent[3] = {a.nx, a.ny, a.nz};
  const int step[3] = {1, a.nx, a.nx * a.ny};
  const int idx[3] = {ix, iy, iz};
  const float pv[3] = {centre(ox, ix, voxel), centre(oy, iy, voxel), centre(oz, iz, voxel)};
  const float dv = D[l];
  const int wv = W[l];
  const float cv[3] = {Cr[l], Cg[l], Cb[l]};
  float gv[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) gv[k] = tsdf_gradient(D, W, a.min_weight, l, idx[k], extent[k], step[k]);
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    if (!(bits & (1 << k))) continue;
    if (row >= max_points) return;          // (rows ascend: every later one is beyond the end too)
    const int m = l + step[k];
    const float dn = D[m];
    const float s = __fdiv_rn(dv, dv - dn);
    float q[3] = {pv[0], pv[1], pv[2]};
    q[k] = pv[k] + (s * voxel);
    const float cn[3] = {Cr[m], Cg[m], Cb[m]};
    float g[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      const float gn = tsdf_gradient(D, W, a.min_weight, m, idx[j] + (j == k ? 1 : 0), extent[j], step[j]);
      g[j] = gv[j] + (s * (gn - gv[j]));
    }
    const float len2 = ((g[0] * g[0]) + (g[1] * g[1])) + (g[2] * g[2]);
    const float nan = __uint_as_float(TS_QNAN);
    float nrm[3] = {nan, nan, nan};
    if (__builtin_isfinite(len2) && len2 > 0.0f) {
      const float len = sqrtf(len2);      // correctly rounded (this toolchain's __fsqrt_rn is the native approximation)
      nrm[0] = __fdiv_rn(g[0], len); nrm[1] = __fdiv_rn(g[1], len); nrm[2] = __fdiv_rn(g[2], len);
    }
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      xyz[row * 3 + j] = q[j];
      rgb[row * 3 + j] = cv[j] + (s * (cn[j] - cv[j]));
      normal[row * 3 + j] = nrm[j];
    }
    weight[row] = min(wv, W[m]);
    ++row;
  }
}

__global__ __launch_bounds__(TS_BLOCK) void tsdf_tail_kernel(const int32_t* __restrict__ block_counts,
                                                             const int32_t* __restrict__ block_base, int blocks, int max_points,
                                                             float* __restrict__ xyz, float* __restrict__ rgb,
                                                             float* __restrict__ normal, int32_t* __restrict__ weight,
                                                             int32_t* __restrict__ num) {
  const long long total = (long long)block_base[blocks - 1] + block_counts[blocks - 1];
  const int K = (int)(total < max_points ? total : max_points);
  const long long row = (long long)blockIdx.x * TS_BLOCK + threadIdx.x;
  if (row == 0) {
    num[0] = K;
    num[1] = (int32_t)total;
    num[3] = total > max_points ? 1 : 0;
  }
  if (row < K || row >= max_points) return;
  const float nan = __uint_as_float(TS_QNAN);
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    xyz[row * 3 + j] = nan;
    rgb[row * 3 + j] = 0.0f;
    normal[row * 3 + j] = nan;
  }
  weight[row] = -1;
}

// ---- raycast: the model view of a virtual pinhole camera --------------------------------------------------------------------
constexpr int RC_TILE = 8;                          // a wave is an 8 x 8 pixel tile: neighbouring rays visit neighbouring voxels
constexpr int RC_WX = 2, RC_WY = 2;                 // ... and a 256-thread workgroup 2 x 2 of them
constexpr int RC_MAX_STEPS = 4096;
constexpr int RC_MAX_DIM = 1 << 24;                 // the inside test compares exact floats up to here

enum { RC_NO_SURFACE = 0, RC_BACK_FACE = 1, RC_HIT = 2, RC_HIT_NO_NORMAL = 3, RC_CODES = 4 };

struct RaycastArgs {
  int n[3], sy, sz;                                 // dims; words to the next voxel along y and z
  int min_weight, n_steps, width, height, clip;
  float top[3];                                     // (float)(n_k - 1)
  float o[3], voxel;
  float rfx, rfy, cx, cy;
  float r[12];
  float near, step;
};

// the ray point of pixel (du, dv) = ((float)u - cx, (float)v - cy) at depth z: camera frame, then common frame
__device__ __forceinline__ void rc_point(const RaycastArgs& a, float du, float dv, float z, float c[3], float p[3]) {
  c[0] = (du * z) * a.rfx;
  c[1] = (dv * z) * a.rfy;
  c[2] = z;
#pragma unroll
  for (int k = 0; k < 3; ++k) p[k] = affine3(a.r + 4 * k, c[0], c[1], c[2]);
}

// the cell of p: its lower corner's linear index and the three fractions; false when p is not inside the box of voxel centres
__device__ __forceinline__ bool rc_cell(const RaycastArgs& a, const float p[3], int& l, float f[3]) {
  bool inside = true;
  int i[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const float g = __fdiv_rn(p[k] - a.o[k], a.voxel) - 0.5f;
    const float fl = floorf(g);
    f[k] = g - fl;
    inside = inside && fl >= 0.0f && (fl + 1.0f) <= a.top[k];      // in float: a NaN fails
    i[k] = inside ? (int)fl : 0;
  }
  l = voxel_index<int>(i[0], i[1], i[2], a.n[0], a.n[1]);
  return inside;
}

__device__ __forceinline__ bool rc_observed(const int32_t* __restrict__ W, const RaycastArgs& a, int l) {
  int w = min(W[l], W[l + 1]);
  w = min(w, min(W[l + a.sy], W[l + a.sy + 1]));
  w = min(w, min(W[l + a.sz], W[l + a.sz + 1]));
  w = min(w, min(W[l + a.sz + a.sy], W[l + a.sz + a.sy + 1]));
  return w >= a.min_weight;
}

// a + (f * (b - a)) along x, then y, then z
__device__ __forceinline__ float rc_trilinear(const float* __restrict__ P, const RaycastArgs& a, int l, const float f[3]) {
  const float d000 = P[l], d100 = P[l + 1], d010 = P[l + a.sy], d110 = P[l + a.sy + 1];
  const float d001 = P[l + a.sz], d101 = P[l + a.sz + 1], d011 = P[l + a.sz + a.sy], d111 = P[l + a.sz + a.sy + 1];
  const float c00 = d000 + (f[0] * (d100 - d000)), c10 = d010 + (f[0] * (d110 - d010));
  const float c01 = d001 + (f[0] * (d101 - d001)), c11 = d011 + (f[0] * (d111 - d011));
  const float c0 = c00 + (f[1] * (c10 - c00)), c1 = c01 + (f[1] * (c11 - c01));
  return c0 + (f[2] * (c1 - c0));
}

// S(p): whether the sample is known, and its value
__device__ __forceinline__ bool rc_sample(const Planes& v, const RaycastArgs& a, const float p[3], float& value) {
  int l;
  float f[3];
  if (!rc_cell(a, p, l, f) || !rc_observed(v.W, a, l)) return false;
  value = rc_trilinear(v.D, a, l, f);
  return true;
}

// the samples [first, last] outside which the ray's point cannot lie inside the box of voxel centres (ray_clip.h, which
// view_gain.hip's march shares)
__device__ __forceinline__ void rc_clip(const RaycastArgs& a, float du, float dv, int& first, int& last) {
  ray_clip(a.r, a.n, a.o, a.voxel, a.near, a.step, a.n_steps, du, dv, a.rfx, a.rfy, first, last);
}

__global__ __launch_bounds__(TS_BLOCK) void tsdf_raycast_kernel(Planes vol, const RaycastArgs a, float* __restrict__ xyz,
                                                                float* __restrict__ normals, float* __restrict__ rgb,
                                                                uint8_t* __restrict__ status, int32_t* __restrict__ counts) {
  __shared__ int s_hist[RC_CODES];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int tiles_x = (a.width + RC_TILE * RC_WX - 1) / (RC_TILE * RC_WX);
  const int bx = (int)(blockIdx.x % (unsigned)tiles_x), by = (int)(blockIdx.x / (unsigned)tiles_x);
  const int u = (bx * RC_WX + (wave % RC_WX)) * RC_TILE + (lane & (RC_TILE - 1));
  const int v = (by * RC_WY + (wave / RC_WX)) * RC_TILE + (lane / RC_TILE);
  const bool active = u < a.width && v < a.height;
  if (tid < RC_CODES) s_hist[tid] = 0;
  __syncthreads();
  const float nan = __uint_as_float(TS_QNAN);
  int code = RC_NO_SURFACE;
  float hit[3] = {nan, nan, nan}, nrm[3] = {nan, nan, nan}, col[3] = {0.0f, 0.0f, 0.0f};
  if (active) {
    const float du = (float)u - a.cx, dv = (float)v - a.cy;
    int first = 0, last = a.n_steps - 1;
    if (a.clip) rc_clip(a, du, dv, first, last);
    bool prev_positive = false;
    float v_prev = 0.0f, z_prev = 0.0f, z_hit = 0.0f;
    for (int i = first; i <= last; ++i) {
      const float z = a.near + ((float)i * a.step);
      float c[3], p[3], value;
      rc_point(a, du, dv, z, c, p);
      if (!rc_sample(vol, a, p, value)) { prev_positive = false; continue; }
      if (value <= 0.0f) {
        code = RC_BACK_FACE;
        if (prev_positive) {
          code = RC_HIT_NO_NORMAL;
          const float s = __fdiv_rn(v_prev, v_prev - value);
          z_hit = z_prev + (s * a.step);
        }
        break;
      }
      prev_positive = value > 0.0f;      // (a NaN value is no previous sample either)
      v_prev = value;
      z_prev = z;
    }
    if (code == RC_HIT_NO_NORMAL) {
      float p[3];
      rc_point(a, du, dv, z_hit, hit, p);
      if (rgb) {
        int l;
        float f[3];
        if (rc_cell(a, p, l, f) && rc_observed(vol.W, a, l)) {
#pragma unroll
          for (int k = 0; k < 3; ++k) col[k] = rc_trilinear(vol.C[k], a, l, f);
        }
      }
      float g[3];
      bool known = true;
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        float q[3] = {p[0], p[1], p[2]};
        float hi = 0.0f, lo = 0.0f;
        q[k] = p[k] + a.voxel;
        known = rc_sample(vol, a, q, hi) && known;
        q[k] = p[k] - a.voxel;
        known = rc_sample(vol, a, q, lo) && known;
        g[k] = hi - lo;
      }
      if (known) {
        float n[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) n[k] = ((a.r[k] * g[0]) + (a.r[4 + k] * g[1])) + (a.r[8 + k] * g[2]);      // R^T
        const float len2 = ((n[0] * n[0]) + (n[1] * n[1])) + (n[2] * n[2]);
        if (__builtin_isfinite(len2) && len2 > 0.0f) {
          const float len = sqrtf(len2);
          n[0] = __fdiv_rn(n[0], len); n[1] = __fdiv_rn(n[1], len); n[2] = __fdiv_rn(n[2], len);
          const float dot = ((n[0] * hit[0]) + (n[1] * hit[1])) + (n[2] * hit[2]);
          const bool flip = dot > 0.0f;
#pragma unroll
          for (int k = 0; k < 3; ++k) nrm[k] = flip ? -n[k] : n[k];
          code = RC_HIT;
        }
      }
    }
    const long long row = (long long)v * a.width + u;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      xyz[row * 3 + k] = hit[k];
      normals[row * 3 + k] = nrm[k];
      if (rgb) rgb[row * 3 + k] = col[k];
    }
    status[row] = (uint8_t)code;
  }
#pragma unroll
  for (int c = 0; c < RC_CODES; ++c) {
    const int n = __popcll(__ballot(active && code == c));
    if (lane == 0 && n != 0) atomicAdd(&s_hist[c], n);
  }
  // one integer atomic per workgroup and code
  __syncthreads();
  if (tid < RC_CODES) {
    const int n = s_hist[tid];
    if (n != 0) atomicAdd(&counts[tid], n);
  }
}

int tsdf_dims(int64_t nx, int64_t ny, int64_t nz) {
  if (nx < 1 || ny < 1 || nz < 1) return REGNET_ERR_SHAPE;
  if (nx > TS_MAX_VOXELS || ny > TS_MAX_VOXELS || nz > TS_MAX_VOXELS || nx * ny > TS_MAX_VOXELS || nx * ny * nz > TS_MAX_VOXELS)
    return REGNET_ERR_UNSUPPORTED;
  return REGNET_OK;
}

// a length in metres given as a double: positive and finite, in float32 too
bool tsdf_length(double v) {
  const float f = (float)v;
  return v > 0.0 && f > 0.0f && f < __builtin_inff();
}

}  // namespace

extern "C" int64_t regnet_tsdf_bytes(int64_t nx, int64_t ny, int64_t nz) {
  return tsdf_dims(nx, ny, nz) == REGNET_OK ? 20 * nx * ny * nz : -1;
}

extern "C" int64_t regnet_tsdf_blocks(int64_t nx, int64_t ny, int64_t nz) {
  return tsdf_dims(nx, ny, nz) == REGNET_OK ? (nx * ny * nz + TS_BLOCK - 1) / TS_BLOCK : -1;
}

extern "C" int64_t regnet_tsdf_integrate_workgroups(int64_t nx, int64_t ny, int64_t nz) {
  if (tsdf_dims(nx, ny, nz) != REGNET_OK) return -1;
  return ((nx + TS_TX - 1) / TS_TX) * ((ny + TS_TY - 1) / TS_TY) * ((nz + TS_TZ - 1) / TS_TZ);
}

extern "C" int regnet_tsdf_reset(void* volume, int64_t nx, int64_t ny, int64_t nz, void* stream) {
  const int bad = tsdf_dims(nx, ny, nz);
  if (bad != REGNET_OK) return bad;
  if (!volume) return REGNET_ERR_NULL;
  const long long n = (long long)(nx * ny * nz);
  hipLaunchKernelGGL(tsdf_reset_kernel, dim3((unsigned)((n + TS_BLOCK - 1) / TS_BLOCK)), dim3(TS_BLOCK), 0, as_stream(stream),
                     planes_of(volume, n), n);
  REGNET_LAUNCH_CHECK();
  return REGNET_OK;
}

extern "C" int regnet_tsdf_integrate_f32(void* volume, int64_t nx, int64_t ny, int64_t nz, const float* origin3, double voxel,
                                         double trunc, int64_t max_weight, const float* xyz, const float* rgb, int64_t width,
                                         int64_t height, const float* intrinsics4, const float* pose12, int32_t* counts,
                                         void* stream) {
  const int bad = tsdf_dims(nx, ny, nz);
  if (bad == REGNET_ERR_SHAPE || width < 1 || height < 1 || max_weight < 1) return REGNET_ERR_SHAPE;
  if (bad != REGNET_OK) return bad;
  if (width > TS_MAX_PIXELS || height > TS_MAX_PIXELS || width * height > TS_MAX_PIXELS) return REGNET_ERR_UNSUPPORTED;
  if (!tsdf_length(voxel) || !tsdf_length(trunc) || !tsdf_length(1.0 / trunc)) return REGNET_ERR_UNSUPPORTED;
  if (!volume || !origin3 || !xyz || !intrinsics4 || !pose12 || !counts) return REGNET_ERR_NULL;
  IntegrateArgs a;
  a.nx = (int)nx; a.ny = (int)ny; a.nz = (int)nz;
  a.tiles_x = (int)((nx + TS_TX - 1) / TS_TX); a.tiles_y = (int)((ny + TS_TY - 1) / TS_TY);
  a.width = (int)width; a.height = (int)height;
  a.max_weight = (int)(max_weight < 0x7FFFFFFF ? max_weight : 0x7FFFFFFF);
  for (int i = 0; i < 3; ++i) a.o[i] = origin3[i];
  a.voxel = (float)voxel; a.trunc = (float)trunc; a.rtrunc = (float)(1.0 / trunc);
  a.fx = intrinsics4[0]; a.fy = intrinsics4[1]; a.cx = intrinsics4[2]; a.cy = intrinsics4[3];
  for (int i = 0; i < 12; ++i) a.r[i] = pose12[i];
  hipStream_t s = as_stream(stream);
  const long long n = (long long)(nx * ny * nz);
  const long long grid = regnet_tsdf_integrate_workgroups(nx, ny, nz);      // at most N <= 2^28
  hipLaunchKernelGGL(tsdf_clear_kernel, dim3(1), dim3(64), 0, s, counts);
  REGNET_LAUNCH_CHECK();
  hipLaunchKernelGGL(tsdf_integrate_kernel, dim3((unsigned)grid), dim3(TS_BLOCK), 0, s, planes_of(volume, n), a, xyz, rgb, counts);
  REGNET_LAUNCH_CHECK();
  return REGNET_OK;
}

extern "C" int regnet_tsdf_count(const void* volume, int64_t nx, int64_t ny, int64_t nz, int64_t min_weight, int32_t* block_counts,
                                 int32_t* num, void* stream) {
  const int bad = tsdf_dims(nx, ny, nz);
  if (bad == REGNET_ERR_SHAPE || min_weight < 1) return REGNET_ERR_SHAPE;
  if (bad != REGNET_OK) return bad;
  if (!volume || !block_counts || !num) return REGNET_ERR_NULL;
  const long long n = (long long)(nx * ny * nz);
  const Planes p = planes_of(const_cast<void*>(volume), n);
  ExtractArgs a;
  a.nx = (int)nx; a.ny = (int)ny; a.nz = (int)nz; a.n = (int)n;
  a.min_weight = (int)(min_weight < 0x7FFFFFFF ? min_weight : 0x7FFFFFFF);
  hipStream_t s = as_stream(stream);
  hipLaunchKernelGGL(tsdf_clear_kernel, dim3(1), dim3(64), 0, s, num);
  REGNET_LAUNCH_CHECK();
  const long long blocks = (n + TS_BLOCK - 1) / TS_BLOCK;
  hipLaunchKernelGGL(tsdf_count_kernel, dim3((unsigned)((blocks + TS_CB - 1) / TS_CB)), dim3(TS_BLOCK), 0, s, p.D, p.W, a,
                     block_counts, num);
  REGNET_LAUNCH_CHECK();
  return REGNET_OK;
}

extern "C" int regnet_tsdf_emit_f32(const void* volume, int64_t nx, int64_t ny, int64_t nz, const float* origin3, double voxel,
                                    int64_t min_weight, const int32_t* block_counts, const int32_t* block_base, int64_t max_points,
                                    float* xyz, float* rgb, float* normal, int32_t* weight, int32_t* num, void* stream) {
  const int bad = tsdf_dims(nx, ny, nz);
  if (bad == REGNET_ERR_SHAPE || min_weight < 1 || max_points < 1) return REGNET_ERR_SHAPE;
  if (bad != REGNET_OK) return bad;
  if (max_points > TS_MAX_POINTS || !tsdf_length(voxel)) return REGNET_ERR_UNSUPPORTED;
  if (!volume || !origin3 || !block_counts || !block_base || !xyz || !rgb || !normal || !weight || !num) return REGNET_ERR_NULL;
  const long long n = (long long)(nx * ny * nz);
  const Planes p = planes_of(const_cast<void*>(volume), n);
  ExtractArgs a;
  a.nx = (int)nx; a.ny = (int)ny; a.nz = (int)nz; a.n = (int)n;
  a.min_weight = (int)(min_weight < 0x7FFFFFFF ? min_weight : 0x7FFFFFFF);
  const int blocks = (int)((n + TS_BLOCK - 1) / TS_BLOCK);
  hipStream_t s = as_stream(stream);
  hipLaunchKernelGGL(tsdf_emit_kernel, dim3((unsigned)blocks), dim3(TS_BLOCK), 0, s, p.D, p.W, p.C[0], p.C[1], p.C[2], a,
                     origin3[0], origin3[1], origin3[2], (float)voxel, block_base, (int)max_points, xyz, rgb, normal, weight);
  REGNET_LAUNCH_CHECK();
  hipLaunchKernelGGL(tsdf_tail_kernel, dim3((unsigned)((max_points + TS_BLOCK - 1) / TS_BLOCK)), dim3(TS_BLOCK), 0, s, block_counts,
                     block_base, blocks, (int)max_points, xyz, rgb, normal, weight, num);
  REGNET_LAUNCH_CHECK();
  return REGNET_OK;
}

extern "C" int regnet_tsdf_raycast_f32(const void* volume, int64_t nx, int64_t ny, int64_t nz, const float* origin3, double voxel,
                                       int64_t min_weight, const float* intrinsics4, const float* pose12, double near, double step,
                                       int64_t n_steps, int64_t width, int64_t height, int clip, float* xyz, float* normals,
                                       float* rgb, uint8_t* status, int32_t* counts, void* stream) {
  const int bad = tsdf_dims(nx, ny, nz);
  if (bad == REGNET_ERR_SHAPE || width < 1 || height < 1 || min_weight < 1 || n_steps < 1) return REGNET_ERR_SHAPE;
  if (bad != REGNET_OK) return bad;
  if (nx > RC_MAX_DIM || ny > RC_MAX_DIM || nz > RC_MAX_DIM) return REGNET_ERR_UNSUPPORTED;
  if (width > TS_MAX_PIXELS || height > TS_MAX_PIXELS || width * height > TS_MAX_PIXELS || n_steps > RC_MAX_STEPS)
    return REGNET_ERR_UNSUPPORTED;
  if (!tsdf_length(voxel) || !tsdf_length(near) || !tsdf_length(step)) return REGNET_ERR_UNSUPPORTED;
  if (!volume || !origin3 || !intrinsics4 || !pose12 || !xyz || !normals || !status || !counts) return REGNET_ERR_NULL;
  RaycastArgs a;
  a.n[0] = (int)nx; a.n[1] = (int)ny; a.n[2] = (int)nz;
  a.sy = (int)nx; a.sz = (int)(nx * ny);
  a.min_weight = (int)(min_weight < 0x7FFFFFFF ? min_weight : 0x7FFFFFFF);
  a.n_steps = (int)n_steps; a.width = (int)width; a.height = (int)height; a.clip = clip != 0;
  for (int k = 0; k < 3; ++k) { a.top[k] = (float)(a.n[k] - 1); a.o[k] = origin3[k]; }
  a.voxel = (float)voxel;
  a.rfx = intrinsics4[0]; a.rfy = intrinsics4[1]; a.cx = intrinsics4[2]; a.cy = intrinsics4[3];
  for (int i = 0; i < 12; ++i) a.r[i] = pose12[i];
  a.near = (float)near; a.step = (float)step;
  hipStream_t s = as_stream(stream);
  const long long n = (long long)(nx * ny * nz);
  const long long grid = ((width + RC_TILE * RC_WX - 1) / (RC_TILE * RC_WX)) * ((height + RC_TILE * RC_WY - 1) / (RC_TILE * RC_WY));
  hipLaunchKernelGGL(tsdf_clear_kernel, dim3(1), dim3(64), 0, s, counts);
  REGNET_LAUNCH_CHECK();
  hipLaunchKernelGGL(tsdf_raycast_kernel, dim3((unsigned)grid), dim3(TS_BLOCK), 0, s, planes_of(const_cast<void*>(volume), n), a,
                     xyz, normals, rgb, status, counts);
  REGNET_LAUNCH_CHECK();
  return REGNET_OK;
}
