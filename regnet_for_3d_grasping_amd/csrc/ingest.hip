// ingest.hip -- the front end of the reference's test.py on the device (gfx950): a raw depth-camera frame becomes the
// network's (N, 6) input without leaving HBM.
//
// test.py:101-129: the frame is moved into the table frame by a rigid 4x4 transform (:104), cropped to the workspace by
// five strict half-space tests on the float64 coordinates (:114-118), the colours are scaled by utils.noise_color's gains
// (utils.py:426-431) and N rows are drawn with np.random.choice (:122-127).  The draws come from numpy's generator
// (np_random_dev.hip consumes the same stream on the device); this file is
//   * the transform + crop as an ORDER-PRESERVING compaction (np.random.choice indexes the cropped list, so its order is part
//     of the contract): per-wave ballots and per-workgroup counts -> one single-workgroup exclusive scan -> placement with
//     mbcnt.  Three short launches, no workgroup ever waits for another;
//   * the gather + colour gain + rounding to float32 of the picked rows (one thread per output row, as dataset.hip);
//   * host code: the LZF decompressor of `DATA binary_compressed` PCD files.
// Built with -ffp-contract=off: every coordinate is ((T[r][0] x + T[r][1] y) + T[r][2] z) + T[r][3] with each product and
// sum individually rounded in float64 -- the order of numpy's / Eigen's 4x4 times (x, y, z, 1) product without FMA.
#include "common.h"

namespace {

constexpr int IG_BLOCK = 256;                 // points per workgroup (4 waves)
constexpr int IG_WAVES = IG_BLOCK / 64;
constexpr int IG_SCAN = 1024;                 // threads of the scan workgroup
constexpr long long IG_MAX_POINTS = 1ll << 21;
constexpr int IG_MAX_BLOCKS = (int)(IG_MAX_POINTS / IG_BLOCK);   // 8192 = IG_SCAN x 8
constexpr int IG_PER_THREAD = IG_MAX_BLOCKS / IG_SCAN;

struct CropArgs {
  double T[12];        // rows 0..2 of the row-major 4x4 transform (the last row is not read: rigid transforms)
  double bound[5];     // x_hi, x_lo, z_hi, y_hi, y_lo  (test.py:114-118, all strict)
  int drop_nonfinite;
};

__device__ __forceinline__ bool finite_f64(double v) { return __builtin_isfinite(v); }

template <typename T>
__device__ __forceinline__ void load_point(const T* __restrict__ xyz, long long i, double& x, double& y, double& z) {
  x = (double)xyz[i * 3 + 0]; y = (double)xyz[i * 3 + 1]; z = (double)xyz[i * 3 + 2];
}

__device__ __forceinline__ void transform_point(const CropArgs& a, double x, double y, double z, double& tx, double& ty,
                                                double& tz) {
  tx = affine3(a.T, x, y, z);
  ty = affine3(a.T + 4, x, y, z);
  tz = affine3(a.T + 8, x, y, z);
}

// pass 1: one ballot per wave (kept for pass 3, so both passes agree by construction) + the workgroup's count
template <typename T>
__global__ __launch_bounds__(IG_BLOCK) void ingest_crop_flag_kernel(const T* __restrict__ xyz, long long M, const CropArgs a,
                                                                    unsigned long long* __restrict__ wave_mask,
                                                                    int* __restrict__ block_count) {
  __shared__ int s_cnt[IG_WAVES];
  const long long i = (long long)blockIdx.x * IG_BLOCK + threadIdx.x;
  bool keep = false;
  if (i < M) {
    double x, y, z, tx, ty, tz;
    load_point(xyz, i, x, y, z);
    transform_point(a, x, y, z, tx, ty, tz);
    keep = tx < a.bound[0] && tx > a.bound[1] && tz < a.bound[2] && ty < a.bound[3] && ty > a.bound[4];
    if (a.drop_nonfinite) keep = keep && finite_f64(x) && finite_f64(y) && finite_f64(z);
  }
  const unsigned long long mask = (unsigned long long)__ballot(keep);
  const int wave = threadIdx.x >> 6;
  if (lane_id() == 0) {
    wave_mask[(long long)blockIdx.x * IG_WAVES + wave] = mask;
    s_cnt[wave] = __popcll(mask);
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    int c = 0;
#pragma unroll
    for (int w = 0; w < IG_WAVES; ++w) c += s_cnt[w];
    block_count[blockIdx.x] = c;
  }
}

// pass 2: exclusive scan of at most IG_MAX_BLOCKS counts by ONE workgroup, in place; the total goes to *count
__global__ __launch_bounds__(IG_SCAN) void ingest_crop_scan_kernel(int* __restrict__ block_count, int blocks,
                                                                   int* __restrict__ count) {
  __shared__ int s_wave[IG_SCAN / 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int v[IG_PER_THREAD];
  int mine = 0;
#pragma unroll
  for (int k = 0; k < IG_PER_THREAD; ++k) {
    const int b = tid * IG_PER_THREAD + k;
    v[k] = b < blocks ? block_count[b] : 0;
    mine += v[k];
  }
  int incl = mine;                                  // inclusive scan inside the wave
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int o = __shfl_up(incl, d, 64);
    if (lane >= d) incl += o;
  }
  if (lane == 63) s_wave[wave] = incl;
  __syncthreads();
  int base = 0;
  for (int w = 0; w < wave; ++w) base += s_wave[w];
  int run = base + incl - mine;
#pragma unroll
  for (int k = 0; k < IG_PER_THREAD; ++k) {
    const int b = tid * IG_PER_THREAD + k;
    if (b < blocks) block_count[b] = run;
    run += v[k];
  }
  if (tid == IG_SCAN - 1) *count = run;
}

// pass 3: placement in input order
template <typename T>
__global__ __launch_bounds__(IG_BLOCK) void ingest_crop_place_kernel(const T* __restrict__ xyz, const T* __restrict__ rgb,
                                                                     long long M, const CropArgs a,
                                                                     const unsigned long long* __restrict__ wave_mask,
                                                                     const int* __restrict__ block_offset,
                                                                     double* __restrict__ kept_xyz64,
                                                                     float* __restrict__ kept_xyz32,
                                                                     double* __restrict__ kept_rgb, int* __restrict__ kept_src) {
  const int wave = threadIdx.x >> 6;
  const unsigned long long* masks = wave_mask + (long long)blockIdx.x * IG_WAVES;
  int before = 0;
#pragma unroll
  for (int w = 0; w < IG_WAVES; ++w) before += w < wave ? __popcll(masks[w]) : 0;
  const unsigned long long mask = masks[wave];
  if (!((mask >> lane_id()) & 1ull)) return;
  const long long i = (long long)blockIdx.x * IG_BLOCK + threadIdx.x;      // (a set bit implies i < M)
  const long long o = (long long)block_offset[blockIdx.x] + before + mbcnt64(mask);
  if (o >= M) return;                                                      // cannot happen; never write out of bounds
  double x, y, z, tx, ty, tz;
  load_point(xyz, i, x, y, z);
  transform_point(a, x, y, z, tx, ty, tz);
  kept_xyz64[o * 3 + 0] = tx; kept_xyz64[o * 3 + 1] = ty; kept_xyz64[o * 3 + 2] = tz;
  kept_xyz32[o * 3 + 0] = (float)tx; kept_xyz32[o * 3 + 1] = (float)ty; kept_xyz32[o * 3 + 2] = (float)tz;
  kept_rgb[o * 3 + 0] = (double)rgb[i * 3 + 0]; kept_rgb[o * 3 + 1] = (double)rgb[i * 3 + 1];
  kept_rgb[o * 3 + 2] = (double)rgb[i * 3 + 2];
  if (kept_src) kept_src[o] = (int)i;
}

template <typename T>
int crop_launch(const T* xyz, const T* rgb, int64_t M, const double* transform, const double* bounds, int drop_nonfinite,
                double* kept_xyz64, float* kept_xyz32, double* kept_rgb, int32_t* kept_src, int32_t* count, void* workspace,
                void* stream) {
  if (M < 0) return REGNET_ERR_SHAPE;
  if (M > IG_MAX_POINTS) return REGNET_ERR_UNSUPPORTED;
  if (!count || !transform || !bounds) return REGNET_ERR_NULL;
  hipStream_t s = as_stream(stream);
  if (M == 0) {
    if (hipMemsetAsync(count, 0, sizeof(int32_t), s) != hipSuccess) return (int)hipGetLastError();
    return REGNET_OK;
  }
  if (!xyz || !rgb || !kept_xyz64 || !kept_xyz32 || !kept_rgb || !workspace) return REGNET_ERR_NULL;
  CropArgs a;
  for (int k = 0; k < 12; ++k) a.T[k] = transform[k];
  for (int k = 0; k < 5; ++k) a.bound[k] = bounds[k];
  a.drop_nonfinite = drop_nonfinite ? 1 : 0;
  const int blocks = (int)((M + IG_BLOCK - 1) / IG_BLOCK);
  unsigned long long* wave_mask = (unsigned long long*)workspace;
  int* block_count = (int*)(wave_mask + (long long)blocks * IG_WAVES);
  hipLaunchKernelGGL(ingest_crop_flag_kernel<T>, dim3(blocks), dim3(IG_BLOCK), 0, s, xyz, (long long)M, a, wave_mask,
                     block_count);
  REGNET_LAUNCH_CHECK();
  hipLaunchKernelGGL(ingest_crop_scan_kernel, dim3(1), dim3(IG_SCAN), 0, s, block_count, blocks, (int*)count);
  REGNET_LAUNCH_CHECK();
  hipLaunchKernelGGL(ingest_crop_place_kernel<T>, dim3(blocks), dim3(IG_BLOCK), 0, s, xyz, rgb, (long long)M, a, wave_mask,
                     block_count, kept_xyz64, kept_xyz32, kept_rgb, (int*)kept_src);
  REGNET_LAUNCH_CHECK();
  return REGNET_OK;
}

// gather + gain + rounding.  RGB64: the float64 array of the real_data branch (the product is a float64 product, rounded to
// float32 by torch.Tensor(pc)); else the float32 record arrays: numpy (>= 2, NEP 50) multiplies a float32 column by a
// float64 scalar IN DOUBLE before rounding back to float32 -- dataset.hip's _noise_color, pinned by tests/golden/s10_ingest.npz.
template <bool RGB64>
__global__ __launch_bounds__(256) void ingest_resample_kernel(const float* __restrict__ xyz, const void* __restrict__ rgb,
                                                              const int* __restrict__ count, long long rows,
                                                              const long long* __restrict__ pick, long long N,
                                                              const double* __restrict__ rand3, float* __restrict__ pc,
                                                              int* __restrict__ bad) {
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  if (t >= N) return;
  long long limit = count ? (long long)*count : rows;
  if (limit > rows) limit = rows;
  const long long j = pick[t];
  float* o = pc + t * 6;
  if (j < 0 || j >= limit) {      // an empty kept list (np.random.choice raises there) or a foreign pick: never read out of bounds
    if (bad) atomicOr(bad, 1);
#pragma unroll
    for (int c = 0; c < 6; ++c) o[c] = 0.0f;
    return;
  }
  o[0] = xyz[j * 3 + 0]; o[1] = xyz[j * 3 + 1]; o[2] = xyz[j * 3 + 2];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const double gain = 1.0 - rand3[c] / 5.0;
    const double v = RGB64 ? ((const double*)rgb)[j * 3 + c] : (double)((const float*)rgb)[j * 3 + c];
    o[3 + c] = (float)(v * gain);
  }
}

}  // namespace

extern "C" int64_t regnet_ingest_crop_workspace_bytes(int64_t M) {
  if (M < 0 || M > IG_MAX_POINTS) return -1;
  const int64_t blocks = (M + IG_BLOCK - 1) / IG_BLOCK;
  return blocks * IG_WAVES * 8 + blocks * 4;
}

extern "C" int regnet_ingest_crop_f32(const float* xyz, const float* rgb, int64_t M, const double* transform,
                                      const double* bounds, int drop_nonfinite, double* kept_xyz64, float* kept_xyz32,
                                      double* kept_rgb, int32_t* kept_src, int32_t* count, void* workspace, void* stream) {
  return crop_launch<float>(xyz, rgb, M, transform, bounds, drop_nonfinite, kept_xyz64, kept_xyz32, kept_rgb, kept_src, count,
                            workspace, stream);
}

extern "C" int regnet_ingest_crop_f64(const double* xyz, const double* rgb, int64_t M, const double* transform,
                                      const double* bounds, int drop_nonfinite, double* kept_xyz64, float* kept_xyz32,
                                      double* kept_rgb, int32_t* kept_src, int32_t* count, void* workspace, void* stream) {
  return crop_launch<double>(xyz, rgb, M, transform, bounds, drop_nonfinite, kept_xyz64, kept_xyz32, kept_rgb, kept_src, count,
                             workspace, stream);
}

extern "C" int regnet_ingest_resample_f32(const float* xyz, const void* rgb, int rgb_is_f64, const int32_t* count, int64_t rows,
                                          const int64_t* pick, int64_t N, const double* rand3, float* pc, int32_t* out_of_range,
                                          void* stream) {
  if (rows < 0 || N < 0) return REGNET_ERR_SHAPE;
  if (N == 0) return REGNET_OK;
  if (!pick || !rand3 || !pc || (rows > 0 && (!xyz || !rgb))) return REGNET_ERR_NULL;
  if ((N + 255) / 256 >= (1ll << 31)) return REGNET_ERR_UNSUPPORTED;
  const dim3 grid((unsigned)((N + 255) / 256));
  if (rgb_is_f64)
    hipLaunchKernelGGL(ingest_resample_kernel<true>, grid, dim3(256), 0, as_stream(stream), xyz, rgb, (const int*)count,
                       (long long)rows, (const long long*)pick, (long long)N, rand3, pc, (int*)out_of_range);
  else
    hipLaunchKernelGGL(ingest_resample_kernel<false>, grid, dim3(256), 0, as_stream(stream), xyz, rgb, (const int*)count,
                       (long long)rows, (const long long*)pick, (long long)N, rand3, pc, (int*)out_of_range);
  REGNET_LAUNCH_CHECK();
  return REGNET_OK;
}

// ---- host: LZF (Marc Lehmann's liblzf format, the codec of PCL's `DATA binary_compressed`) -------------------------------
// A control byte c < 32 starts a literal run of c + 1 bytes; otherwise a back reference: length (c >> 5) + 2, extended by the
// next byte when c >> 5 == 7, at distance ((c & 31) << 8 | next byte) + 1 behind the write position (runs may overlap it).
extern "C" int64_t regnet_lzf_decompress(const uint8_t* in, int64_t in_len, uint8_t* out, int64_t out_cap) {
  if (in_len < 0 || out_cap < 0) return REGNET_ERR_SHAPE;
  if ((in_len > 0 && !in) || (out_cap > 0 && !out)) return REGNET_ERR_NULL;
  int64_t ip = 0, op = 0;
  while (ip < in_len) {
    const unsigned ctrl = in[ip++];
    if (ctrl < 32) {
      const int64_t run = (int64_t)ctrl + 1;
      if (ip + run > in_len || op + run > out_cap) return REGNET_ERR_SHAPE;
      for (int64_t k = 0; k < run; ++k) out[op++] = in[ip++];
    } else {
      int64_t len = ctrl >> 5;
      if (len == 7) {
        if (ip >= in_len) return REGNET_ERR_SHAPE;
        len += in[ip++];
      }
      if (ip >= in_len) return REGNET_ERR_SHAPE;
      const int64_t ref = op - (int64_t)(((ctrl & 31u) << 8) | in[ip++]) - 1;
      len += 2;
      if (ref < 0 || op + len > out_cap) return REGNET_ERR_SHAPE;
      for (int64_t k = 0; k < len; ++k) out[op++] = out[ref + k];
    }
  }
  return op;
}
