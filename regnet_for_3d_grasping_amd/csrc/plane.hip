// plane.hip -- the dominant support plane of one camera frame on the device (gfx950): the step that replaces the hard-coded
// camera pose of ingest.table_frame_transform() by a calibration made on the frame itself (table_plane.py).
//
// RANSAC with everything that decides pinned (DESIGN.md par. 5, include/regnet_hip.h).  Built with -ffp-contract=off: every
// product, sum and difference below is an individually rounded binary32 operation in the written order, so a numpy float32
// restatement (tests/plane_reference.py) gives the same bits.  The points are the float32 values of the input (a float64 input
// is rounded once, to nearest); a row with a non-finite float32 coordinate takes no part.
//
//   * plane_hypotheses_kernel: one thread per hypothesis h.  Three rows drawn with splitmix64 over the counter
//     seed * 2^32 + (3 h + k) * 8 + r (slot k, attempt r = 0..7, row = ((z >> 32) * M) >> 32, the first attempt that hits a
//     finite row), n = (p1 - p0) x (p2 - p0), nn = ((nx nx) + (ny ny)) + (nz nz), the validity and gate flags; writes the
//     (H, 8) table [n, p0, nn, flag] and the count kernel's parameter rows [n, p0, (t t) nn or -1, 0], and zeroes the counts.
//   * plane_count_kernel, the hot path: a workgroup holds 2048 points in registers (8 per lane) and walks its share of the
//     hypotheses; the parameters come from LDS as wave-wide broadcasts; per hypothesis and point slot one 64-bit ballot and a
//     scalar popcount; per-workgroup counts in an LDS table; one integer atomic per hypothesis and workgroup.
//   * plane_select_kernel: ONE workgroup: counts of ineligible hypotheses -> -1, argmax with ties to the lower index, zeroes
//     the moments.
//   * plane_moments_kernel: re-tests every point against the winner, writes the (M) uint8 inlier mask and reduces the ten
//     float64 moments per workgroup -> one float64 atomic per sum and workgroup (tgemm.hip's statistics pattern).
//   * plane_moments_partial_kernel + plane_moments_sum_kernel (regnet_plane_moments_det_*): the ten moments over a given mask in
//     one fixed order, without atomics -- what estimate_plane refits from, so that one cloud gives one plane bit for bit.
// No workgroup waits for another: the four launches are ordered by the stream.  Integer atomics only for everything that is
// compared exactly; every other result is written by plain vector stores.
#include "common.h"

namespace {

constexpr long long PL_MAX_POINTS = 1ll << 21;
constexpr int PL_MAX_H = 4096;
constexpr int PL_BLOCK = 256;
constexpr int PL_PPL = 8;                           // points per lane
constexpr int PL_TILE = PL_BLOCK * PL_PPL;          // points per workgroup
constexpr int PL_HCHUNK = 128;                      // hypotheses per count workgroup (64 when H is no multiple of 128)
constexpr int PL_ATTEMPTS = 8;
constexpr int PL_SELECT_THREADS = 1024;
constexpr int PL_SELECT_PER_THREAD = PL_MAX_H / PL_SELECT_THREADS;

struct PlaneArgs {
  unsigned long long seed;
  float t2, lo2, hi2;      // float32 products t t, lo lo, hi hi
  float c2;                // cos^2(max tilt), evaluated in float64 on the host and rounded once
  float ux, uy, uz;
  int use_tilt;
};

__device__ __forceinline__ unsigned long long splitmix64(unsigned long long x) {
  unsigned long long z = x + 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

// row i as float32; false (and NaN coordinates, which fail every inlier test) when one of them is not finite
template <typename T>
__device__ __forceinline__ bool load_row(const T* __restrict__ xyz, long long i, float& x, float& y, float& z) {
  x = (float)xyz[i * 3 + 0]; y = (float)xyz[i * 3 + 1]; z = (float)xyz[i * 3 + 2];
  const bool ok = __builtin_isfinite(x) && __builtin_isfinite(y) && __builtin_isfinite(z);
  if (!ok) x = y = z = __builtin_nanf("");
  return ok;
}

template <typename T>
__global__ __launch_bounds__(64) void plane_hypotheses_kernel(const T* __restrict__ xyz, long long M, int H, const PlaneArgs a,
                                                              float* __restrict__ table, float* __restrict__ params,
                                                              int* __restrict__ counts) {
  const int h = blockIdx.x * 64 + threadIdx.x;
  if (h >= H) return;
  float p[3][3];
  bool filled = true;
  for (int k = 0; k < 3; ++k) {
    bool got = false;
    p[k][0] = p[k][1] = p[k][2] = 0.0f;
    for (int r = 0; r < PL_ATTEMPTS && !got; ++r) {
      const unsigned long long c = (a.seed << 32) + (unsigned long long)((3 * h + k) * 8 + r);
      const unsigned long long row = ((splitmix64(c) >> 32) * (unsigned long long)M) >> 32;      // < M
      float x, y, z;
      if (load_row(xyz, (long long)row, x, y, z)) {
        p[k][0] = x; p[k][1] = y; p[k][2] = z;
        got = true;
      }
    }
    filled = filled && got;
  }
  float out[8] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
  float thr = -1.0f;
  if (filled) {
    const float ax = p[1][0] - p[0][0], ay = p[1][1] - p[0][1], az = p[1][2] - p[0][2];
    const float bx = p[2][0] - p[0][0], by = p[2][1] - p[0][1], bz = p[2][2] - p[0][2];
    const float nx = (ay * bz) - (az * by), ny = (az * bx) - (ax * bz), nz = (ax * by) - (ay * bx);
    const float nn = dot3(nx, ny, nz, nx, ny, nz);
    const bool valid = nn > 1e-12f && nn < __builtin_inff();
    const float g = dot3(p[0][0], p[0][1], p[0][2], nx, ny, nz);
    const float gg = g * g;
    bool eligible = (a.lo2 * nn <= gg) && (gg <= a.hi2 * nn);
    if (a.use_tilt) {
      const float d = dot3(nx, ny, nz, a.ux, a.uy, a.uz);
      const float uu = dot3(a.ux, a.uy, a.uz, a.ux, a.uy, a.uz);
      eligible = eligible && (d * d >= (a.c2 * nn) * uu);
    }
    out[0] = nx; out[1] = ny; out[2] = nz;
    out[3] = p[0][0]; out[4] = p[0][1]; out[5] = p[0][2];
    out[6] = nn;
    out[7] = valid ? (eligible ? 2.0f : 1.0f) : 0.0f;
    if (valid && eligible) thr = a.t2 * nn;
  }
  float4* t4 = reinterpret_cast<float4*>(table + (long long)h * 8);
  t4[0] = make_float4(out[0], out[1], out[2], out[3]);
  t4[1] = make_float4(out[4], out[5], out[6], out[7]);
  float4* p4 = reinterpret_cast<float4*>(params + (long long)h * 8);
  p4[0] = make_float4(out[0], out[1], out[2], out[3]);
  p4[1] = make_float4(out[4], out[5], thr, 0.0f);          // thr = -1: no point is an inlier (s s >= 0, a NaN fails)
  counts[h] = 0;
}

// grid (point tiles, H / hc): 10 VALU operations per point-plane test (3 sub, 4 mul, 2 add, 1 compare)
template <typename T>
__global__ __launch_bounds__(PL_BLOCK) void plane_count_kernel(const T* __restrict__ xyz, long long M, int hc,
                                                               const float* __restrict__ params, int* __restrict__ counts) {
  __shared__ float4 s_par[PL_HCHUNK * 2];
  __shared__ int s_cnt[PL_HCHUNK];
  const int tid = threadIdx.x;
  const int h0 = blockIdx.y * hc;
  const float4* src = reinterpret_cast<const float4*>(params) + (long long)h0 * 2;
  for (int i = tid; i < hc * 2; i += PL_BLOCK) s_par[i] = src[i];
  if (tid < hc) s_cnt[tid] = 0;
  float px[PL_PPL], py[PL_PPL], pz[PL_PPL];
  const long long base = (long long)blockIdx.x * PL_TILE + tid;
#pragma unroll
  for (int j = 0; j < PL_PPL; ++j) {
    const long long i = base + (long long)j * PL_BLOCK;
    px[j] = py[j] = pz[j] = __builtin_nanf("");
    if (i < M) load_row(xyz, i, px[j], py[j], pz[j]);
  }
  __syncthreads();
  const bool first = lane_id() == 0;
  for (int h = 0; h < hc; ++h) {
    const float4 A = s_par[2 * h], B = s_par[2 * h + 1];        // nx ny nz qx | qy qz thr -
    int c = 0;
#pragma unroll
    for (int j = 0; j < PL_PPL; ++j) {
      const float dx = px[j] - A.w, dy = py[j] - B.x, dz = pz[j] - B.y;
      const float s = dot3(dx, dy, dz, A.x, A.y, A.z);
      c += __popcll(__ballot(s * s <= B.z));
    }
    if (first && c != 0) atomicAdd(&s_cnt[h], c);
  }
  __syncthreads();
  if (tid < hc) {
    const int c = s_cnt[tid];
    if (c != 0) atomicAdd(&counts[h0 + tid], c);
  }
}

__global__ __launch_bounds__(PL_SELECT_THREADS) void plane_select_kernel(const float* __restrict__ table, int H,
                                                                         int* __restrict__ counts, int* __restrict__ winner,
                                                                         double* __restrict__ moments) {
  __shared__ long long s_key[PL_SELECT_THREADS / 64];
  const int tid = threadIdx.x;
  // key = count * 2^32 + (2^32 - 1 - h): the larger count, then the lower index
  long long best = -1;
#pragma unroll
  for (int k = 0; k < PL_SELECT_PER_THREAD; ++k) {
    const int h = tid + k * PL_SELECT_THREADS;
    if (h < H) {
      if (table[(long long)h * 8 + 7] == 2.0f) {
        const long long key = ((long long)counts[h] << 32) | (long long)(0xffffffffu - (unsigned)h);
        best = key > best ? key : best;
      } else {
        counts[h] = -1;
      }
    }
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    const long long o = __shfl_xor(best, d, 64);
    best = o > best ? o : best;
  }
  if (lane_id() == 0) s_key[tid >> 6] = best;
  __syncthreads();
  if (tid == 0) {
#pragma unroll
    for (int w = 1; w < PL_SELECT_THREADS / 64; ++w) best = s_key[w] > best ? s_key[w] : best;
    const int count = best < 0 ? -1 : (int)(best >> 32);
    const bool found = count >= 3;
    winner[0] = found ? (int)(0xffffffffu - (unsigned)(best & 0xffffffffll)) : -1;
    winner[1] = found ? count : 0;
  }
  if (tid < 10) moments[tid] = 0.0;
}

template <typename T>
__global__ __launch_bounds__(PL_BLOCK) void plane_moments_kernel(const T* __restrict__ xyz, long long M, int H,
                                                                 const float* __restrict__ params,
                                                                 const int* __restrict__ winner, uint8_t* __restrict__ inlier,
                                                                 double* __restrict__ moments) {
  __shared__ double s_part[PL_BLOCK / 64][10];
  const int tid = threadIdx.x;
  const int w = winner[0];
  float nx = 0.0f, ny = 0.0f, nz = 0.0f, qx = 0.0f, qy = 0.0f, qz = 0.0f, thr = -1.0f;
  if (w >= 0 && w < H) {
    const float4 A = reinterpret_cast<const float4*>(params)[(long long)w * 2];
    const float4 B = reinterpret_cast<const float4*>(params)[(long long)w * 2 + 1];
    nx = A.x; ny = A.y; nz = A.z; qx = A.w; qy = B.x; qz = B.y; thr = B.z;
  }
  double acc[10];
#pragma unroll
  for (int k = 0; k < 10; ++k) acc[k] = 0.0;
  const long long base = (long long)blockIdx.x * PL_TILE + tid;
#pragma unroll 2
  for (int j = 0; j < PL_PPL; ++j) {
    const long long i = base + (long long)j * PL_BLOCK;
    if (i < M) {
      float fx, fy, fz;
      load_row(xyz, i, fx, fy, fz);
      const float dx = fx - qx, dy = fy - qy, dz = fz - qz;
      const float s = dot3(dx, dy, dz, nx, ny, nz);
      const bool in = s * s <= thr;
      inlier[i] = in ? 1 : 0;
      if (in) {
        const double x = (double)fx, y = (double)fy, z = (double)fz;      // the products are exact in float64
        acc[0] += 1.0; acc[1] += x; acc[2] += y; acc[3] += z;
        acc[4] += x * x; acc[5] += x * y; acc[6] += x * z; acc[7] += y * y; acc[8] += y * z; acc[9] += z * z;
      }
    }
  }
#pragma unroll
  for (int k = 0; k < 10; ++k) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) acc[k] += __shfl_xor(acc[k], d, 64);
  }
  if (lane_id() == 0) {
#pragma unroll
    for (int k = 0; k < 10; ++k) s_part[tid >> 6][k] = acc[k];
  }
  __syncthreads();
  if (tid < 10) {
    double n = 0.0, v = 0.0;
#pragma unroll
    for (int wv = 0; wv < PL_BLOCK / 64; ++wv) { n += s_part[wv][0]; v += s_part[wv][tid]; }
    if (n != 0.0) unsafeAtomicAdd(&moments[tid], v);
  }
}

// The ten moments once more, in ONE fixed order (regnet_plane_moments_det_*): a workgroup reduces its 2048 points over the given
// mask exactly as plane_moments_kernel does (per-lane order, shuffle tree, waves in order) but leaves its partial row in the
// workspace instead of adding it atomically; plane_moments_sum_kernel, one workgroup, adds the rows in a fixed order.
template <typename T>
__global__ __launch_bounds__(PL_BLOCK) void plane_moments_partial_kernel(const T* __restrict__ xyz, long long M,
                                                                         const uint8_t* __restrict__ inlier,
                                                                         double* __restrict__ partial) {
  __shared__ double s_part[PL_BLOCK / 64][10];
  const int tid = threadIdx.x;
  double acc[10];
#pragma unroll
  for (int k = 0; k < 10; ++k) acc[k] = 0.0;
  const long long base = (long long)blockIdx.x * PL_TILE + tid;
#pragma unroll 2
  for (int j = 0; j < PL_PPL; ++j) {
    const long long i = base + (long long)j * PL_BLOCK;
    if (i < M && inlier[i] != 0) {
      float fx, fy, fz;
      if (load_row(xyz, i, fx, fy, fz)) {
        const double x = (double)fx, y = (double)fy, z = (double)fz;
        acc[0] += 1.0; acc[1] += x; acc[2] += y; acc[3] += z;
        acc[4] += x * x; acc[5] += x * y; acc[6] += x * z; acc[7] += y * y; acc[8] += y * z; acc[9] += z * z;
      }
    }
  }
#pragma unroll
  for (int k = 0; k < 10; ++k) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) acc[k] += __shfl_xor(acc[k], d, 64);
  }
  if (lane_id() == 0) {
#pragma unroll
    for (int k = 0; k < 10; ++k) s_part[tid >> 6][k] = acc[k];
  }
  __syncthreads();
  if (tid < 10) {
    double v = 0.0;
#pragma unroll
    for (int wv = 0; wv < PL_BLOCK / 64; ++wv) v += s_part[wv][tid];
    partial[(long long)blockIdx.x * 10 + tid] = v;
  }
}

__global__ __launch_bounds__(64) void plane_moments_sum_kernel(const double* __restrict__ partial, int rows,
                                                               double* __restrict__ moments) {
  const int tid = threadIdx.x;
  if (tid < 10) {
    double v = 0.0;
    for (int r = 0; r < rows; ++r) v += partial[(long long)r * 10 + tid];      // ascending tile order
    moments[tid] = v;
  }
}

template <typename T>
int plane_moments_det_launch(const T* xyz, int64_t M, const uint8_t* inlier, double* moments, void* workspace, void* stream) {
  if (M < 0) return REGNET_ERR_SHAPE;
  if (M > PL_MAX_POINTS) return REGNET_ERR_UNSUPPORTED;
  if (!moments || !workspace) return REGNET_ERR_NULL;
  if (M > 0 && (!xyz || !inlier)) return REGNET_ERR_NULL;
  hipStream_t s = as_stream(stream);
  const int tiles = (int)((M + PL_TILE - 1) / PL_TILE);
  if (tiles > 0) {
    hipLaunchKernelGGL(plane_moments_partial_kernel<T>, dim3((unsigned)tiles), dim3(PL_BLOCK), 0, s, xyz, (long long)M, inlier,
                       (double*)workspace);
    REGNET_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(plane_moments_sum_kernel, dim3(1), dim3(64), 0, s, (const double*)workspace, tiles, moments);
  REGNET_LAUNCH_CHECK();
  return REGNET_OK;
}

template <typename T>
int plane_launch(const T* xyz, int64_t M, int64_t H, uint64_t seed, float threshold, float range_lo, float range_hi,
                 const float* up_hint, float cos2_tilt, float* hypotheses, int32_t* counts, uint8_t* inlier, double* moments,
                 int32_t* winner, void* workspace, int stages, void* stream) {
  if (M < 0 || H <= 0 || H % 64 != 0) return REGNET_ERR_SHAPE;
  if (M > PL_MAX_POINTS || H > PL_MAX_H) return REGNET_ERR_UNSUPPORTED;
  if (!hypotheses || !counts || !moments || !winner || !workspace) return REGNET_ERR_NULL;
  if (M > 0 && (!xyz || !inlier)) return REGNET_ERR_NULL;
  if (stages < 1 || stages > 15) return REGNET_ERR_SHAPE;
  hipStream_t s = as_stream(stream);
  PlaneArgs a;
  a.seed = seed;
  a.t2 = threshold * threshold;
  a.lo2 = range_lo * range_lo;
  a.hi2 = range_hi * range_hi;
  a.c2 = cos2_tilt;
  a.use_tilt = up_hint ? 1 : 0;
  a.ux = up_hint ? up_hint[0] : 0.0f; a.uy = up_hint ? up_hint[1] : 0.0f; a.uz = up_hint ? up_hint[2] : 0.0f;
  float* params = (float*)workspace;
  if (M == 0) {        // no row to draw: every hypothesis invalid, winner -1
    if (hipMemsetAsync(hypotheses, 0, (size_t)H * 8 * sizeof(float), s) != hipSuccess) return (int)hipGetLastError();
    if (hipMemsetAsync(counts, 0xff, (size_t)H * sizeof(int32_t), s) != hipSuccess) return (int)hipGetLastError();
    if (hipMemsetAsync(moments, 0, 10 * sizeof(double), s) != hipSuccess) return (int)hipGetLastError();
    if (hipMemsetAsync(winner, 0xff, sizeof(int32_t), s) != hipSuccess) return (int)hipGetLastError();
    if (hipMemsetAsync(winner + 1, 0, sizeof(int32_t), s) != hipSuccess) return (int)hipGetLastError();
    return REGNET_OK;
  }
  const int tiles = (int)((M + PL_TILE - 1) / PL_TILE);
  const int hc = (H % PL_HCHUNK == 0) ? PL_HCHUNK : 64;
  if (stages & 1) {
    hipLaunchKernelGGL(plane_hypotheses_kernel<T>, dim3((unsigned)(H / 64)), dim3(64), 0, s, xyz, (long long)M, (int)H, a,
                       hypotheses, params, (int*)counts);
    REGNET_LAUNCH_CHECK();
  }
  if (stages & 2) {
    hipLaunchKernelGGL(plane_count_kernel<T>, dim3((unsigned)tiles, (unsigned)(H / hc)), dim3(PL_BLOCK), 0, s, xyz,
                       (long long)M, hc, (const float*)params, (int*)counts);
    REGNET_LAUNCH_CHECK();
  }
  if (stages & 4) {
    hipLaunchKernelGGL(plane_select_kernel, dim3(1), dim3(PL_SELECT_THREADS), 0, s, (const float*)hypotheses, (int)H,
                       (int*)counts, (int*)winner, moments);
    REGNET_LAUNCH_CHECK();
  }
  if (stages & 8) {
    hipLaunchKernelGGL(plane_moments_kernel<T>, dim3((unsigned)tiles), dim3(PL_BLOCK), 0, s, xyz, (long long)M, (int)H,
                       (const float*)params, (const int*)winner, inlier, moments);
    REGNET_LAUNCH_CHECK();
  }
  return REGNET_OK;
}

}  // namespace

extern "C" int64_t regnet_plane_workspace_bytes(int64_t M, int64_t H) {
  if (M < 0 || M > PL_MAX_POINTS || H <= 0 || H % 64 != 0 || H > PL_MAX_H) return -1;
  return H * 8 * (int64_t)sizeof(float);
}

extern "C" int regnet_plane_estimate_f32(const float* xyz, int64_t M, int64_t H, uint64_t seed, float threshold, float range_lo,
                                         float range_hi, const float* up_hint, float cos2_tilt, float* hypotheses,
                                         int32_t* counts, uint8_t* inlier, double* moments, int32_t* winner, void* workspace,
                                         int stages, void* stream) {
  return plane_launch<float>(xyz, M, H, seed, threshold, range_lo, range_hi, up_hint, cos2_tilt, hypotheses, counts, inlier,
                             moments, winner, workspace, stages, stream);
}

extern "C" int regnet_plane_estimate_f64(const double* xyz, int64_t M, int64_t H, uint64_t seed, float threshold, float range_lo,
                                         float range_hi, const float* up_hint, float cos2_tilt, float* hypotheses,
                                         int32_t* counts, uint8_t* inlier, double* moments, int32_t* winner, void* workspace,
                                         int stages, void* stream) {
  return plane_launch<double>(xyz, M, H, seed, threshold, range_lo, range_hi, up_hint, cos2_tilt, hypotheses, counts, inlier,
                              moments, winner, workspace, stages, stream);
}

extern "C" int64_t regnet_plane_moments_det_workspace_bytes(int64_t M) {
  if (M < 0 || M > PL_MAX_POINTS) return -1;
  const int64_t tiles = (M + PL_TILE - 1) / PL_TILE;
  return (tiles > 0 ? tiles : 1) * 10 * (int64_t)sizeof(double);
}

extern "C" int regnet_plane_moments_det_f32(const float* xyz, int64_t M, const uint8_t* inlier, double* moments, void* workspace,
                                            void* stream) {
  return plane_moments_det_launch<float>(xyz, M, inlier, moments, workspace, stream);
}

extern "C" int regnet_plane_moments_det_f64(const double* xyz, int64_t M, const uint8_t* inlier, double* moments, void* workspace,
                                            void* stream) {
  return plane_moments_det_launch<double>(xyz, M, inlier, moments, workspace, stream);
}
