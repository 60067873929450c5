// outlier.hip -- outlier removal over one cloud on the device (gfx950): the saturating radius count (open3d's
// remove_radius_outlier, the reference's PointCloud.remove_outliers), the mean distance to the k nearest neighbours and the
// cloud statistics of open3d / PCL's statistical outlier removal.  Built with -ffp-contract=off: d2 is sqdist3, three
// individually rounded products summed left to right, so tests/outlier_reference.py decides every pair the same way; the grid
// (grid.h) only decides WHICH pairs are evaluated.  Contract: include/regnet_hip.h, DESIGN.md par. 5.
//
//   outlier_init_kernel    the outputs of the rows outside the graph (-1, the quiet NaN); the graph rows (mask set,
//                          coordinates finite) compacted (wave-aggregated atomicAdd, any order): excluded rows never reach the grid
//   build_grid             over the compacted rows, cell edge >= radius, the row count read on the device
//   outlier_radius_kernel  a wave per graph row over the rows of the cells overlapping its ball, 64 candidates a step: ballot +
//                          popcount, and the wave leaves as soon as it has min_neighbours (the count saturates there)
//   outlier_knn_kernel     a wave per graph row, the same walk; the k best d2 live one per lane in ascending order, a step's
//                          candidates below the current k-th value are inserted one at a time
//   outlier_stats_kernel   one workgroup: n, the mean and the two-pass deviation of the mean distances in float64, fixed order
// Neither search depends on the order in which the candidates are met: a count, and the multiset of the k smallest values.
#include "grid.h"

namespace {

constexpr unsigned OL_QNAN = 0x7fc00000u;
constexpr int OL_STATS_WG = 1024;

struct OutlierLayout {   // byte offsets into the workspace
  long long cnt, src, cxyz, grid, total;
};

__host__ inline OutlierLayout outlier_layout(long long N) {
  auto up = [](long long b) { return (b + 15) / 16 * 16; };
  OutlierLayout L;
  L.cnt = 0;                        // int32[4]: graph rows
  L.src = 16;                       // int32[N]: compacted row -> source row
  L.cxyz = L.src + up(N * 4);       // float[3 N]: compacted coordinates
  L.grid = L.cxyz + up(N * 12);
  L.total = L.grid + up(grid_slab_bytes(N));
  return L;
}

__device__ __forceinline__ bool outlier_finite3(float x, float y, float z) {
  return fabsf(x) < __builtin_inff() && fabsf(y) < __builtin_inff() && fabsf(z) < __builtin_inff();   // (NaN fails)
}

// (cluster.hip's compaction, restated: the per-row outputs differ)
__global__ __launch_bounds__(256) void outlier_init_kernel(const float* __restrict__ xyz, const uint8_t* __restrict__ mask, int N,
                                                      int* __restrict__ cnt, int* __restrict__ src, float* __restrict__ cxyz,
                                                      int* __restrict__ count, unsigned* __restrict__ mean_dist) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  float x = 0.f, y = 0.f, z = 0.f;
  bool valid = false;
  if (i < N) {
    x = xyz[(int64_t)i * 3]; y = xyz[(int64_t)i * 3 + 1]; z = xyz[(int64_t)i * 3 + 2];
    valid = (mask == nullptr || mask[i] != 0) && outlier_finite3(x, y, z);
    if (!valid) {
      count[i] = -1;
      if (mean_dist) mean_dist[i] = OL_QNAN;
    }
  }
  const int c = wave_append(valid, &cnt[0]);
  if (valid) {
    src[c] = i;
    cxyz[(int64_t)c * 3] = x; cxyz[(int64_t)c * 3 + 1] = y; cxyz[(int64_t)c * 3 + 2] = z;
  }
}

struct OlWalk {   // the cells overlapping the ball of one graph row
  int x0, x1, y0, y1, z0, z1;
};

__device__ __forceinline__ OlWalk outlier_walk(const GridHeader& H, float qx, float qy, float qz, float radius) {
  const float pad = radius * 1.0001f + H.eps + 4e-6f * fmaxf(fmaxf(fabsf(qx), fabsf(qy)), fabsf(qz));   // conservative cell range of the ball
  OlWalk w;
  w.x0 = cell_coord(qx - pad, H.lo[0], H.inv_h, H.dim[0]); w.x1 = cell_coord(qx + pad, H.lo[0], H.inv_h, H.dim[0]);
  w.y0 = cell_coord(qy - pad, H.lo[1], H.inv_h, H.dim[1]); w.y1 = cell_coord(qy + pad, H.lo[1], H.inv_h, H.dim[1]);
  w.z0 = cell_coord(qz - pad, H.lo[2], H.inv_h, H.dim[2]); w.z1 = cell_coord(qz + pad, H.lo[2], H.inv_h, H.dim[2]);
  return w;
}

__global__ __launch_bounds__(256) void outlier_radius_kernel(const float* __restrict__ cxyz, const int* __restrict__ src,
                                                        const int* __restrict__ cnt, int N, float R2, float radius,
                                                        int min_nb, const char* __restrict__ slab, int* __restrict__ count) {
  const int lane = lane_id();
  const long long c = blockIdx.x * 4ll + (threadIdx.x >> 6);
  if (c >= min(N, cnt[0])) return;   // wave-uniform
  const GridHeader H = *reinterpret_cast<const GridHeader*>(slab);
  const int* cell_start = grid_cell_start(const_cast<char*>(slab));
  const float4* sorted = grid_sorted(const_cast<char*>(slab));
  const float qx = cxyz[c * 3], qy = cxyz[c * 3 + 1], qz = cxyz[c * 3 + 2];
  const OlWalk w = outlier_walk(H, qx, qy, qz, radius);
  int n = 0;
  for (int z = w.z0; z <= w.z1 && n < min_nb; ++z)
    for (int y = w.y0; y <= w.y1 && n < min_nb; ++y) {
      const int row = (z * H.dim[1] + y) * H.dim[0];
      const int beg = cell_start[row + w.x0], end = cell_start[row + w.x1 + 1];   // the x-run of cells is contiguous
      for (int k0 = beg; k0 < end; k0 += 64) {
        const int k = k0 + lane;
        bool hit = false;
        if (k < end) {
          const float4 p = sorted[k];
          hit = sqdist3(qx, qy, qz, p.x, p.y, p.z) <= R2 && __float_as_int(p.w) != (int)c;   // by row: a duplicate counts
        }
        n += (int)__popcll(__ballot(hit));
        if (n >= min_nb) break;   // saturated: count[i] = min(n, min_nb) is decided
      }
    }
  if (lane == 0) count[src[c]] = min(n, min_nb);
}

__global__ __launch_bounds__(256) void outlier_knn_kernel(const float* __restrict__ cxyz, const int* __restrict__ src,
                                                     const int* __restrict__ cnt, int N, float R2, float radius, int K,
                                                     const char* __restrict__ slab, float* __restrict__ mean_dist,
                                                     int* __restrict__ found) {
  const int lane = lane_id();
  const long long c = blockIdx.x * 4ll + (threadIdx.x >> 6);
  if (c >= min(N, cnt[0])) return;   // wave-uniform
  const GridHeader H = *reinterpret_cast<const GridHeader*>(slab);
  const int* cell_start = grid_cell_start(const_cast<char*>(slab));
  const float4* sorted = grid_sorted(const_cast<char*>(slab));
  const float qx = cxyz[c * 3], qy = cxyz[c * 3 + 1], qz = cxyz[c * 3 + 2];
  const OlWalk w = outlier_walk(H, qx, qy, qz, radius);
  const float inf = __builtin_inff();
  float best = inf;   // lane l: the l-th smallest d2 so far, +inf beyond those found and for lanes >= K
  float kth = inf;    // lane K - 1's value
  int n = 0;
  for (int z = w.z0; z <= w.z1; ++z)
    for (int y = w.y0; y <= w.y1; ++y) {
      const int row = (z * H.dim[1] + y) * H.dim[0];
      const int beg = cell_start[row + w.x0], end = cell_start[row + w.x1 + 1];
      for (int k0 = beg; k0 < end; k0 += 64) {
        const int k = k0 + lane;
        float d2 = inf;
        bool hit = false;
        if (k < end) {
          const float4 p = sorted[k];
          d2 = sqdist3(qx, qy, qz, p.x, p.y, p.z);
          hit = d2 <= R2 && __float_as_int(p.w) != (int)c;
        }
        n += (int)__popcll(__ballot(hit));
        // a candidate equal to the k-th value would replace an equal value: only the multiset counts, so it is skipped
        bool live = hit && d2 < kth;
        for (uint64_t todo = __ballot(live); todo != 0ull; todo = __ballot(live)) {
          const int leader = __builtin_ctzll(todo);
          const float cand = __shfl(d2, leader, 64);
          const int pos = (int)__popcll(__ballot(best <= cand));   // best ascends: the lanes below pos keep their value
          const float below = __shfl_up(best, 1, 64);
          best = lane < pos ? best : (lane == pos ? cand : below);
          if (lane >= K) best = inf;
          kth = __shfl(best, K - 1, 64);
          live = live && lane != leader && d2 < kth;
        }
      }
    }
  // S: the float64 sum of the correctly rounded float32 roots in ascending order of d2, one addition after the other
  const int f = min(n, K);
  const float root = sqrtf(best);
  double S = 0.0;
  if (f == K)
    for (int l = 0; l < K; ++l) S += (double)__shfl(root, l, 64);
  if (lane == 0) {
    const int i = src[c];
    found[i] = f;
    mean_dist[i] = f == K ? (float)(S / (double)K) : __uint_as_float(OL_QNAN);
  }
}

// One workgroup.  Fixed order: thread t adds rows t, t + WG, ... one after the other, then a tree over the threads in LDS.
__device__ __forceinline__ double outlier_block_sum(double v, double* red) {
  const int t = threadIdx.x;
  __syncthreads();   // (red is reused)
  red[t] = v;
  __syncthreads();
  for (int off = OL_STATS_WG / 2; off > 0; off >>= 1) {
    if (t < off) red[t] = red[t] + red[t + off];
    __syncthreads();
  }
  return red[0];
}

__global__ __launch_bounds__(OL_STATS_WG) void outlier_stats_kernel(const float* __restrict__ mean_dist, const int* __restrict__ found,
                                                               int N, int K, double ratio, double* __restrict__ stats) {
  __shared__ double red[OL_STATS_WG];
  const int t = threadIdx.x;
  double cnt = 0.0, sum = 0.0;
  for (int i = t; i < N; i += OL_STATS_WG)
    if (found[i] == K) { cnt += 1.0; sum += (double)mean_dist[i]; }
  const double n = outlier_block_sum(cnt, red);
  const double total = outlier_block_sum(sum, red);
  const double mu = total / n;   // (0 / 0: NaN without a row)
  double dev = 0.0;
  for (int i = t; i < N; i += OL_STATS_WG)
    if (found[i] == K) { const double d = (double)mean_dist[i] - mu; dev += d * d; }
  const double ss = outlier_block_sum(dev, red);
  if (t == 0) {
    const double sigma = n >= 2.0 ? sqrt(ss / (n - 1.0)) : __longlong_as_double(0x7ff8000000000000ll);
    const double scaled = ratio * sigma;
    stats[0] = n;
    stats[1] = mu;
    stats[2] = sigma;
    stats[3] = n >= 2.0 ? (double)(float)(mu + scaled) : (double)__builtin_inff();
  }
}

bool outlier_radius_ok(float r) { return r > 0.f && r < __builtin_inff(); }

// the compaction and the grid, shared by the two searches
int outlier_prepare(const float* xyz, const uint8_t* mask, int64_t N, float radius, int32_t* count, float* mean_dist, char* ws,
               const OutlierLayout& L, hipStream_t st) {
  int* cnt = (int*)(ws + L.cnt);
  hipError_t e = hipMemsetAsync(cnt, 0, 16, st);
  if (e != hipSuccess) return (int)e;
  hipLaunchKernelGGL(outlier_init_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, st, xyz, mask, (int)N, cnt,
                     (int*)(ws + L.src), (float*)(ws + L.cxyz), (int*)count, (unsigned*)mean_dist);
  REGNET_LAUNCH_CHECK();
  return build_grid((const float*)(ws + L.cxyz), 0, 1, 3, 1, N, radius, ws + L.grid, st, cnt);
}

}  // namespace

extern "C" int64_t regnet_outlier_workspace_bytes(int64_t N) {
  if (N < 0 || N >= (int64_t)1 << 31) return -1;   // the limits of the launch
  return outlier_layout(N).total;
}

extern "C" int regnet_outlier_radius_f32(const float* xyz, const uint8_t* mask, int64_t N, float radius, int64_t min_neighbours,
                                         int32_t* count, void* workspace, void* stream) {
  if (N < 0) return REGNET_ERR_SHAPE;
  if (N >= (int64_t)1 << 31 || min_neighbours < 1 || !outlier_radius_ok(radius)) return REGNET_ERR_UNSUPPORTED;
  if (N == 0) return REGNET_OK;
  if (!xyz || !count || !workspace) return REGNET_ERR_NULL;
  hipStream_t st = as_stream(stream);
  const OutlierLayout L = outlier_layout(N);
  char* ws = (char*)workspace;
  int rc = outlier_prepare(xyz, mask, N, radius, count, nullptr, ws, L, st);
  if (rc) return rc;
  const int mn = (int)(min_neighbours > N ? N : min_neighbours);   // (a row has at most N - 1 neighbours: never reached)
  hipLaunchKernelGGL(outlier_radius_kernel, dim3((unsigned)((N + 3) / 4)), dim3(256), 0, st, (const float*)(ws + L.cxyz),
                     (const int*)(ws + L.src), (const int*)(ws + L.cnt), (int)N, radius * radius, radius, mn,
                     (const char*)(ws + L.grid), (int*)count);
  REGNET_LAUNCH_CHECK();
  return REGNET_OK;
}

extern "C" int regnet_outlier_knn_f32(const float* xyz, const uint8_t* mask, int64_t N, int64_t k, float max_radius,
                                      float* mean_dist, int32_t* found, void* workspace, void* stream) {
  if (N < 0) return REGNET_ERR_SHAPE;
  if (N >= (int64_t)1 << 31 || k < 1 || k > 64 || !outlier_radius_ok(max_radius)) return REGNET_ERR_UNSUPPORTED;
  if (N == 0) return REGNET_OK;
  if (!xyz || !mean_dist || !found || !workspace) return REGNET_ERR_NULL;
  hipStream_t st = as_stream(stream);
  const OutlierLayout L = outlier_layout(N);
  char* ws = (char*)workspace;
  int rc = outlier_prepare(xyz, mask, N, max_radius, found, mean_dist, ws, L, st);
  if (rc) return rc;
  hipLaunchKernelGGL(outlier_knn_kernel, dim3((unsigned)((N + 3) / 4)), dim3(256), 0, st, (const float*)(ws + L.cxyz),
                     (const int*)(ws + L.src), (const int*)(ws + L.cnt), (int)N, max_radius * max_radius, max_radius, (int)k,
                     (const char*)(ws + L.grid), mean_dist, (int*)found);
  REGNET_LAUNCH_CHECK();
  return REGNET_OK;
}

extern "C" int regnet_outlier_stats_f64(const float* mean_dist, const int32_t* found, int64_t N, int64_t k, double ratio,
                                        double* stats, void* stream) {
  if (N < 0) return REGNET_ERR_SHAPE;
  if (N >= (int64_t)1 << 31 || k < 1 || k > 64 || !(ratio >= 0.0) || !(ratio < (double)__builtin_inff())) return REGNET_ERR_UNSUPPORTED;
  if (!stats || (N > 0 && (!mean_dist || !found))) return REGNET_ERR_NULL;
  hipLaunchKernelGGL(outlier_stats_kernel, dim3(1), dim3(OL_STATS_WG), 0, as_stream(stream), mean_dist, (const int*)found, (int)N,
                     (int)k, ratio, stats);
  REGNET_LAUNCH_CHECK();
  return REGNET_OK;
}
