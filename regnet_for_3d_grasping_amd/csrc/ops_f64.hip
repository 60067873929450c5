// ops_f64.hip -- the float64 operators of pn2_ext / dgcnn_ext (gfx950).
//
// The reference dispatches every native operator on float32 AND float64 (AT_DISPATCH_FLOATING_TYPES).  The float32
// path of this library is the tuned one (geometry.hip, grid.hip, gather.hip); this translation unit is the float64
// path of the forwards: the same semantics with double coordinates / features, written for correctness first.  No
// float32 data is read here.  The float64 backwards are deterministic and live in scatter.hip with the float32
// deterministic ones: the same sort plan and the same segment-sum kernels, instantiated for double.
//
// Reference behaviour restated (relative to multi_model/utils/pn2_utils/):
//   FPS         csrc/sampling_kernel.cu:47-117      ball query  csrc/ball_query_kernel.cu:31-74
//   3-NN        csrc/interpolate_kernel.cu:28-77    group       csrc/grouping_kernel.cu:29-149
//   interpolate csrc/interpolate_kernel.cu:134-282  gather_knn  functions/csrc/gather_knn_kernel.cu:27-153
//
// Built with -ffp-contract=off (csrc/build.py): the indices depend on individually rounded distances
// ((dx*dx) + (dy*dy)) + (dz*dz), and the interpolation sums add individually rounded products.
#include "common.h"

__device__ __forceinline__ double sqdist3_f64(double ax, double ay, double az, double bx, double by, double bz) {
  double dx = ax - bx, dy = ay - by, dz = az - bz;
  double xx = dx * dx, yy = dy * dy, zz = dz * dz;
  double s = xx + yy;
  return s + zz;
}

// =====================================================================================
// Furthest point sampling
// =====================================================================================
// The reference's launch, literally: RB = get_block(N) (a power of two, 16 <= RB <= 512) threads per scene; thread t
// scans points t, t + RB, ... keeping its FIRST strict maximum (starting from 0 with the previous pick's index), then
// a tree over the lanes keeps the lower lane on equality.  The tree's upper levels go through LDS, the last six inside
// the first wave through cross-lane moves (lane t reads lane t + off: the same pairs).  The running distances live in
// the caller's workspace (B x N doubles).
#define FPS64_MAX 512

__global__ __launch_bounds__(FPS64_MAX) void fps_f64_kernel(const double* __restrict__ xyz, int64_t sb, int64_t sc,
                                                             int64_t sn, int N, int M, int64_t* __restrict__ index,
                                                             double* __restrict__ temp_all) {
  __shared__ double sd[FPS64_MAX];
  __shared__ int si[FPS64_MAX];
  __shared__ int s_cur;
  const int b = blockIdx.x, t = threadIdx.x, RB = blockDim.x;
  const double* px = xyz + (int64_t)b * sb;
  const double* py = px + sc;
  const double* pz = py + sc;
  double* temp = temp_all + (int64_t)b * N;
  int64_t* out = index + (int64_t)b * M;
  for (int j = t; j < N; j += RB) temp[j] = -1.0;   // sampling_kernel.cu:142 (only this thread touches temp[j])
  if (t == 0) out[0] = 0;
  int cur = 0;
  for (int i = 1; i < M; ++i) {
    const double x1 = px[(int64_t)cur * sn], y1 = py[(int64_t)cur * sn], z1 = pz[(int64_t)cur * sn];
    double best = 0.0;
    int besti = cur;
    for (int j = t; j < N; j += RB) {
      double d = sqdist3_f64(px[(int64_t)j * sn], py[(int64_t)j * sn], pz[(int64_t)j * sn], x1, y1, z1);
      const double last = temp[j];
      if (last > d || last < 0) temp[j] = d;   // sampling_kernel.cu:84-88
      else d = last;
      if (d > best) { best = d; besti = j; }
    }
    sd[t] = best;
    si[t] = besti;
    __syncthreads();
    for (int off = RB / 2; off >= 64; off >>= 1) {
      if (t < off && sd[t] < sd[t + off]) { sd[t] = sd[t + off]; si[t] = si[t + off]; }
      __syncthreads();
    }
    if (t < 64) {
      double v = sd[t];
      int vi = si[t];
      for (int off = (RB < 64 ? RB : 64) / 2; off > 0; off >>= 1) {
        const double ov = __shfl_down(v, off, 64);
        const int oi = __shfl_down(vi, off, 64);
        if (v < ov) { v = ov; vi = oi; }
      }
      if (t == 0) { s_cur = vi; out[i] = vi; }
    }
    __syncthreads();
    cur = s_cur;
  }
}

static int64_t ref_block(int64_t n) {   // sampling_kernel.cu:32-40 + the switch at :148-165 (at least 16)
  int cnt = 0;
  int64_t x = n - 1;
  while (x > 0) { x >>= 1; ++cnt; }
  int64_t b = (int64_t)1 << cnt;
  if (b > FPS64_MAX) b = FPS64_MAX;
  return b < 16 ? 16 : b;
}

extern "C" int64_t regnet_fps_f64_workspace_bytes(int64_t B, int64_t N, int64_t M) {
  (void)M;
  if (B <= 0 || N <= 0) return 0;
  return B * N * (int64_t)sizeof(double);
}

extern "C" int regnet_fps_f64(const double* xyz, int64_t sb, int64_t sc, int64_t sn, int64_t B, int64_t N, int64_t M,
                              int64_t* index, double* workspace, void* stream) {
  if (M <= 0 || N < M || B < 0) return REGNET_ERR_SHAPE;
  if (N >= (int64_t)1 << 30 || B > 65535) return REGNET_ERR_UNSUPPORTED;
  if (B == 0) return REGNET_OK;
  if (!xyz || !index || !workspace) return REGNET_ERR_NULL;
  hipLaunchKernelGGL(fps_f64_kernel, dim3((unsigned)B), dim3((unsigned)ref_block(N)), 0, as_stream(stream), xyz, sb, sc,
                     sn, (int)N, (int)M, index, workspace);
  REGNET_LAUNCH_CHECK();
  return REGNET_OK;
}

// =====================================================================================
// Ball query
// =====================================================================================
// A wave per centroid, 64 points per step: ballot of the in-radius lanes, in-order compaction with mbcnt, stop once K
// members are found.  Slots count..K-1 repeat the first member (the reference pre-fills all K slots with it), or 0
// when the ball is empty.
#define BQ64_WAVES 4

__global__ __launch_bounds__(BQ64_WAVES * 64) void ball_query_f64_kernel(
    const double* __restrict__ xyz, int64_t sb, int64_t sc, int64_t sn, const double* __restrict__ cent, int64_t cb,
    int64_t cc, int64_t cn, int N1, int N2, double r2, int K, int64_t* __restrict__ index, int64_t* __restrict__ count) {
  const int b = blockIdx.y;
  const int m = blockIdx.x * BQ64_WAVES + (int)(threadIdx.x >> 6);
  if (m >= N2) return;   // wave-uniform
  const int lane = lane_id();
  const double* px = xyz + (int64_t)b * sb;
  const double* py = px + sc;
  const double* pz = py + sc;
  const double* c = cent + (int64_t)b * cb + (int64_t)m * cn;
  const double x1 = c[0], y1 = c[cc], z1 = c[2 * cc];
  int64_t* out = index + ((int64_t)b * N2 + m) * K;
  int cnt = 0, first = 0;
  for (int j0 = 0; j0 < N1 && cnt < K; j0 += 64) {
    const int j = j0 + lane;
    bool hit = false;
    if (j < N1) {
      // point minus centroid (ball_query_kernel.cu:60)
      const double d = sqdist3_f64(px[(int64_t)j * sn], py[(int64_t)j * sn], pz[(int64_t)j * sn], x1, y1, z1);
      hit = d < r2;
    }
    const uint64_t mask = (uint64_t)__ballot(hit);
    if (mask == 0) continue;
    if (cnt == 0) first = j0 + __ffsll((unsigned long long)mask) - 1;
    const int pos = cnt + mbcnt64(mask);
    if (hit && pos < K) out[pos] = j;
    cnt += __popcll(mask);
  }
  if (cnt > K) cnt = K;
  for (int k = cnt + lane; k < K; k += 64) out[k] = first;
  if (lane == 0) count[(int64_t)b * N2 + m] = cnt;
}

extern "C" int regnet_ball_query_f64(const double* xyz, int64_t sb, int64_t sc, int64_t sn, const double* centroids,
                                     int64_t cb, int64_t cc, int64_t cn, int64_t B, int64_t N1, int64_t N2,
                                     float radius, int64_t K, int64_t* index, int64_t* count, void* stream) {
  if (K <= 0 || B < 0 || N1 < 0 || N2 < 0) return REGNET_ERR_SHAPE;
  if (N1 >= (int64_t)1 << 31 || N2 >= (int64_t)1 << 31 || K >= (int64_t)1 << 20 || B > 65535)
    return REGNET_ERR_UNSUPPORTED;
  if (B == 0 || N2 == 0) return REGNET_OK;
  if (!centroids || !index || !count || (N1 > 0 && !xyz)) return REGNET_ERR_NULL;
  // the reference's radius is a C++ float (ball_query_kernel.cu:90): widened to double, squared in double
  const double r = (double)radius;
  const double r2 = r * r;
  dim3 grid((unsigned)((N2 + BQ64_WAVES - 1) / BQ64_WAVES), (unsigned)B);
  hipLaunchKernelGGL(ball_query_f64_kernel, grid, dim3(BQ64_WAVES * 64), 0, as_stream(stream), xyz, sb, sc, sn,
                     centroids, cb, cc, cn, (int)N1, (int)N2, r2, (int)K, index, count);
  REGNET_LAUNCH_CHECK();
  return REGNET_OK;
}

// =====================================================================================
// 3-NN search
// =====================================================================================
// One thread per query; keys stream through LDS in tiles of NN64_T (every lane reads the same address: broadcast).
// The reference's initial state {1e40, 0, 0} / {-1, 0, 0} (interpolate_kernel.cu:49-50) is kept as it is -- 1e40 is
// finite in double -- and the sorted insertion uses strict <, so the earlier key wins ties.
#define NN64_T 256

__global__ __launch_bounds__(NN64_T) void three_nn_f64_kernel(const double* __restrict__ q, int64_t qb, int64_t qc,
                                                              int64_t qn, const double* __restrict__ key, int64_t kb,
                                                              int64_t kc, int64_t kn, int N1, int N2,
                                                              int64_t* __restrict__ index, double* __restrict__ dist2) {
  __shared__ double kx[NN64_T], ky[NN64_T], kz[NN64_T];
  const int b = blockIdx.y;
  const int i = blockIdx.x * NN64_T + threadIdx.x;
  const bool live = i < N1;
  double x1 = 0.0, y1 = 0.0, z1 = 0.0;
  if (live) {
    const double* p = q + (int64_t)b * qb + (int64_t)i * qn;
    x1 = p[0]; y1 = p[qc]; z1 = p[2 * qc];
  }
  const double* k0 = key + (int64_t)b * kb;
  double md0 = 1e40, md1 = 0.0, md2 = 0.0;
  int mi0 = -1, mi1 = 0, mi2 = 0;
  for (int base = 0; base < N2; base += NN64_T) {
    const int n = min(NN64_T, N2 - base);
    __syncthreads();
    if ((int)threadIdx.x < n) {
      const double* p = k0 + (int64_t)(base + threadIdx.x) * kn;
      kx[threadIdx.x] = p[0]; ky[threadIdx.x] = p[kc]; kz[threadIdx.x] = p[2 * kc];
    }
    __syncthreads();
    for (int t = 0; t < n; ++t) {
      const double d = sqdist3_f64(x1, y1, z1, kx[t], ky[t], kz[t]);   // query minus key (interpolate_kernel.cu:56)
      const int j = base + t;
      if (d < md0) { md2 = md1; mi2 = mi1; md1 = md0; mi1 = mi0; md0 = d; mi0 = j; }
      else if (d < md1) { md2 = md1; mi2 = mi1; md1 = d; mi1 = j; }
      else if (d < md2) { md2 = d; mi2 = j; }
    }
  }
  if (live) {
    const int64_t o = ((int64_t)b * N1 + i) * 3;
    index[o] = mi0; index[o + 1] = mi1; index[o + 2] = mi2;
    dist2[o] = md0; dist2[o + 1] = md1; dist2[o + 2] = md2;
  }
}

extern "C" int regnet_three_nn_f64(const double* query, int64_t qb, int64_t qc, int64_t qn, const double* key,
                                   int64_t kb, int64_t kc, int64_t kn, int64_t B, int64_t N1, int64_t N2,
                                   int64_t* index, double* dist2, void* stream) {
  if (N2 < 3 || B < 0 || N1 < 0) return REGNET_ERR_SHAPE;
  if (N1 >= (int64_t)1 << 31 || N2 >= (int64_t)1 << 31 || B > 65535) return REGNET_ERR_UNSUPPORTED;
  if (B == 0 || N1 == 0) return REGNET_OK;
  if (!query || !key || !index || !dist2) return REGNET_ERR_NULL;
  dim3 grid((unsigned)((N1 + NN64_T - 1) / NN64_T), (unsigned)B);
  hipLaunchKernelGGL(three_nn_f64_kernel, grid, dim3(NN64_T), 0, as_stream(stream), query, qb, qc, qn, key, kb, kc, kn,
                     (int)N1, (int)N2, index, dist2);
  REGNET_LAUNCH_CHECK();
  return REGNET_OK;
}

// =====================================================================================
// Gathers (forward of group_points / gather_knn / interpolate)
// =====================================================================================
#define G64_T 256
#define G64_CH 16

static inline bool g64_dims_ok(int64_t B, int64_t C) { return B <= 65535 && (C + G64_CH - 1) / G64_CH <= 65535; }

// out[b, c, e] = in[b, c, index[b, e]]; an index outside [0, N1) reads as 0 (the reference asserts)
__global__ __launch_bounds__(G64_T) void group_fwd_f64_kernel(const double* __restrict__ in, int64_t sb, int64_t sc,
                                                              int64_t sn, const int64_t* __restrict__ index, int C,
                                                              int N1, int64_t NK, double* __restrict__ out) {
  const int b = blockIdx.z;
  const int64_t e = (int64_t)blockIdx.x * G64_T + threadIdx.x;
  if (e >= NK) return;
  const int64_t j = index[(int64_t)b * NK + e];
  const bool ok = j >= 0 && j < N1;
  const int cbeg = blockIdx.y * G64_CH, cend = min(C, cbeg + G64_CH);
  const double* src = in + (int64_t)b * sb + (ok ? j : 0) * sn;
  double* dst = out + ((int64_t)b * C) * NK + e;
  for (int c = cbeg; c < cend; ++c) dst[(int64_t)c * NK] = ok ? src[(int64_t)c * sc] : 0.0;
}

// out[b, c, n] = ((+0 + x0 w0) + x1 w1) + x2 w2 (interpolate_kernel.cu:165-170); an index outside [0, M) reads as 0
__global__ __launch_bounds__(G64_T) void interp_fwd_f64_kernel(const double* __restrict__ in, int64_t sb, int64_t sc,
                                                               int64_t sm, const int64_t* __restrict__ index,
                                                               const double* __restrict__ weight, int C, int M, int N,
                                                               double* __restrict__ out) {
  const int b = blockIdx.z;
  const int n = blockIdx.x * G64_T + threadIdx.x;
  if (n >= N) return;
  const int64_t o = ((int64_t)b * N + n) * 3;
  int64_t j[3];
  double w[3];
  bool ok[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    j[k] = index[o + k];
    w[k] = weight[o + k];
    ok[k] = j[k] >= 0 && j[k] < M;
  }
  const int cbeg = blockIdx.y * G64_CH, cend = min(C, cbeg + G64_CH);
  const double* src = in + (int64_t)b * sb;
  double* dst = out + ((int64_t)b * C) * N + n;
  for (int c = cbeg; c < cend; ++c) {
    const double* s = src + (int64_t)c * sc;
    double acc = 0.0;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const double x = ok[k] ? s[j[k] * sm] : 0.0;
      const double p = x * w[k];
      acc = acc + p;
    }
    dst[(int64_t)c * N] = acc;
  }
}

extern "C" int regnet_group_points_fwd_f64(const double* input, int64_t sb, int64_t sc, int64_t sn,
                                           const int64_t* index, int64_t B, int64_t C, int64_t N1, int64_t N2,
                                           int64_t K, double* out, void* stream) {
  if (B < 0 || C < 0 || N1 < 0 || N2 < 0 || K < 0) return REGNET_ERR_SHAPE;
  const int64_t NK = N2 * K;
  if (B == 0 || C == 0 || NK == 0) return REGNET_OK;
  if (!g64_dims_ok(B, C) || N1 >= (int64_t)1 << 31) return REGNET_ERR_UNSUPPORTED;
  if (!input || !index || !out) return REGNET_ERR_NULL;
  dim3 grid((unsigned)((NK + G64_T - 1) / G64_T), (unsigned)((C + G64_CH - 1) / G64_CH), (unsigned)B);
  hipLaunchKernelGGL(group_fwd_f64_kernel, grid, dim3(G64_T), 0, as_stream(stream), input, sb, sc, sn, index, (int)C,
                     (int)N1, NK, out);
  REGNET_LAUNCH_CHECK();
  return REGNET_OK;
}

extern "C" int regnet_interpolate_fwd_f64(const double* input, int64_t sb, int64_t sc, int64_t sm,
                                          const int64_t* index, const double* weight, int64_t B, int64_t C, int64_t M,
                                          int64_t N, double* out, void* stream) {
  if (B < 0 || C < 0 || M < 0 || N < 0) return REGNET_ERR_SHAPE;
  if (B == 0 || C == 0 || N == 0) return REGNET_OK;
  if (M == 0) return REGNET_ERR_SHAPE;
  if (!g64_dims_ok(B, C) || N >= (int64_t)1 << 31 || M >= (int64_t)1 << 31) return REGNET_ERR_UNSUPPORTED;
  if (!input || !index || !weight || !out) return REGNET_ERR_NULL;
  dim3 grid((unsigned)((N + G64_T - 1) / G64_T), (unsigned)((C + G64_CH - 1) / G64_CH), (unsigned)B);
  hipLaunchKernelGGL(interp_fwd_f64_kernel, grid, dim3(G64_T), 0, as_stream(stream), input, sb, sc, sm, index, weight,
                     (int)C, (int)M, (int)N, out);
  REGNET_LAUNCH_CHECK();
  return REGNET_OK;
}

extern "C" int regnet_gather_knn_fwd_f64(const double* input, int64_t sb, int64_t sc, int64_t sn, const int64_t* index,
                                         int64_t B, int64_t C, int64_t N, int64_t NI, int64_t K, double* out,
                                         void* stream) {
  return regnet_group_points_fwd_f64(input, sb, sc, sn, index, B, C, N, NI, K, out, stream);
}
