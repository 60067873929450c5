// det.hip -- the float32 kernels of the deterministic mode (torch.use_deterministic_algorithms), gfx950.
//
// The default float32 backwards of group_points / interpolate / gather_knn (gather.hip) and of the pooled region feature
// (region.hip: scatter_max_grad) add with float atomics in whatever order the hardware runs them.  Here every destination
// adds its contributions in one fixed order, so a training iteration gives the same bits run after run:
//
//   segment sums   -- group / gather_knn / interpolate: each destination element is the sum of its contributions in
//                     ascending flattened source position (m*K + k, n*3 + k), sequentially from +0.0; interpolate adds the
//                     product g*w rounded to float32 (the bits of np.add.at on float32 arrays).  The segments come from the
//                     sort plan of ops_f64.hip (regnet_scatter_plan: per scene, the source positions of every destination,
//                     ascending), which depends on the indices alone: one plan serves every backward of one table.
//   scatter_max    -- grad[arg[r][f]][f] += dy[r][f] in ascending r per channel, onto the value already there.
//
// Built with -ffp-contract=off (csrc/build.py): no product is fused into its addition.
#include "common.h"
#include "scatter_plan.h"

// ---- segment sums, LDS-staged ------------------------------------------------------------------------------------------
// A workgroup owns `cpb` channels of one scene.  It stages the gradient rows of its channels in LDS, a chunk of source
// slots at a time (one coalesced read of the gradient from HBM), and each thread walks the segments of its destinations
// through the chunk: a segment lists ascending source positions, so the part of it inside a chunk is a contiguous run
// that follows the part inside the previous chunk.  With several chunks the per-destination running sums and segment
// cursors live in LDS between chunks; with one chunk they stay in registers.
// Source slot: group / gather_knn (unweighted) the position p itself, at (p / inner) * s_hi + (p % inner) * s_lo;
// interpolate (weighted, inner = 3) the grad_out column p / 3, at (p / 3) * s_hi.
#define DSEG_T 1024
#define DSEG_LDS_FLOATS 36864   // 144 KB
#define DSEG_CH 8               // channels per workgroup at most
#define DSEG_MIN_CHUNK 4096     // below this many staged slots per chunk: the global-memory kernel

template <bool WEIGHTED>
__global__ __launch_bounds__(DSEG_T) void det_segsum_lds_kernel(const float* __restrict__ go, int64_t sb, int64_t sc,
                                                                int64_t s_hi, int64_t s_lo, int inner, int dense,
                                                                const float* __restrict__ weight, int C, int R, int64_t L,
                                                                int NS, int chunk, int cpb, const int* __restrict__ off,
                                                                const int* __restrict__ perm, float* __restrict__ gi) {
  extern __shared__ float sm[];
  float* rows = sm;                          // [cpb][chunk]
  float* acc = sm + cpb * chunk;             // [cpb][R]   (several chunks only)
  int* cur = (int*)(acc + cpb * R);          // [R]
  const int b = blockIdx.y, t = threadIdx.x;
  const int c0 = blockIdx.x * cpb, nc = min(cpb, C - c0);
  const int* o = off + (int64_t)b * (R + 1);
  const int* pm = perm + (int64_t)b * L;
  const float* wt = WEIGHTED ? weight + (int64_t)b * L : nullptr;
  const float* src = go + (int64_t)b * sb + (int64_t)c0 * sc;
  const bool multi = NS > chunk;
  if (multi) {
    for (int n = t; n < R; n += DSEG_T) {
      cur[n] = o[n];
      for (int c = 0; c < nc; ++c) acc[c * R + n] = 0.f;
    }
  }
  for (int s0 = 0; s0 < NS; s0 += chunk) {
    const int ns = min(chunk, NS - s0);
    __syncthreads();
    for (int i = t; i < nc * ns; i += DSEG_T) {
      const int c = i / ns, s = i - c * ns, slot = s0 + s;
      int64_t a;
      if (WEIGHTED) a = (int64_t)slot * s_hi;   // grad_out column slot
      else if (dense) a = slot;                 // row-major (rows, inner): position p itself
      else {
        const int hi = slot / inner;
        a = (int64_t)hi * s_hi + (int64_t)(slot - hi * inner) * s_lo;
      }
      rows[c * chunk + s] = src[(int64_t)c * sc + a];
    }
    __syncthreads();
    const int send = s0 + ns;
    for (int n = t; n < R; n += DSEG_T) {
      int i = multi ? cur[n] : o[n];
      const int end = o[n + 1];
      float a[DSEG_CH];
#pragma unroll
      for (int c = 0; c < DSEG_CH; ++c) a[c] = (multi && c < nc) ? acc[c * R + n] : 0.f;
      for (; i < end; ++i) {
        const int p = pm[i];
        const int slot = WEIGHTED ? p / 3 : p;
        if (slot >= send) break;
        const float* r = rows + (slot - s0);
        if (WEIGHTED) {
          const float w = wt[p];
#pragma unroll
          for (int c = 0; c < DSEG_CH; ++c)
            if (c < nc) {
              const float v = r[c * chunk] * w;
              a[c] = a[c] + v;
            }
        } else {
#pragma unroll
          for (int c = 0; c < DSEG_CH; ++c)
            if (c < nc) a[c] = a[c] + r[c * chunk];
        }
      }
      if (multi) {
        cur[n] = i;
#pragma unroll
        for (int c = 0; c < DSEG_CH; ++c)
          if (c < nc) acc[c * R + n] = a[c];
      } else {
        float* dst = gi + ((int64_t)b * C + c0) * R + n;
#pragma unroll
        for (int c = 0; c < DSEG_CH; ++c)
          if (c < nc) dst[(int64_t)c * R] = a[c];
      }
    }
  }
  if (multi) {
    __syncthreads();
    float* dst = gi + ((int64_t)b * C + c0) * R;
    for (int i = t; i < nc * R; i += DSEG_T) dst[i] = acc[i];
  }
}

// ---- segment sums from global memory (destination counts whose state does not fit in LDS) -------------------------------
// A thread per destination walks its segment in order, DSEG_G_CH channels at a time; the grid runs the destinations of one
// channel block together so that their scattered reads share the cached gradient rows.
#define DSEG_G_T 256
#define DSEG_G_CH 4

template <bool WEIGHTED>
__global__ __launch_bounds__(DSEG_G_T) void det_segsum_global_kernel(const float* __restrict__ go, int64_t sb,
                                                                     int64_t sc, int64_t s_hi, int64_t s_lo, int inner,
                                                                     const float* __restrict__ weight, int C, int R,
                                                                     int64_t L, const int* __restrict__ off,
                                                                     const int* __restrict__ perm,
                                                                     float* __restrict__ gi) {
  const int b = blockIdx.z;
  const int n = blockIdx.x * DSEG_G_T + threadIdx.x;
  if (n >= R) return;
  const int c0 = blockIdx.y * DSEG_G_CH, nc = min(DSEG_G_CH, C - c0);
  const int* o = off + (int64_t)b * (R + 1);
  const int* pm = perm + (int64_t)b * L;
  const float* src = go + (int64_t)b * sb + (int64_t)c0 * sc;
  float a[DSEG_G_CH];
#pragma unroll
  for (int c = 0; c < DSEG_G_CH; ++c) a[c] = 0.f;
  const int end = o[n + 1];
  for (int i = o[n]; i < end; ++i) {
    const int p = pm[i];
    const int hi = p / inner, lo = p - hi * inner;
    const float* e = src + (int64_t)hi * s_hi + (WEIGHTED ? 0 : (int64_t)lo * s_lo);
    const float w = WEIGHTED ? weight[(int64_t)b * L + p] : 1.f;
#pragma unroll
    for (int c = 0; c < DSEG_G_CH; ++c)
      if (c < nc) {
        const float g = e[(int64_t)c * sc];
        if (WEIGHTED) {
          const float v = g * w;
          a[c] = a[c] + v;
        } else {
          a[c] = a[c] + g;
        }
      }
  }
  float* dst = gi + ((int64_t)b * C + c0) * R + n;
#pragma unroll
  for (int c = 0; c < DSEG_G_CH; ++c)
    if (c < nc) dst[(int64_t)c * R] = a[c];
}

// LDS layout of det_segsum_lds_kernel for (R destinations, NS slots): channels per workgroup and slots per chunk, or
// false when it does not fit
static bool lds_layout(int64_t B, int64_t C, int64_t R, int64_t NS, int* cpb_out, int* chunk_out) {
  // one chunk: cpb rows of NS slots, state in registers
  int cpb = (int)(DSEG_LDS_FLOATS / (NS > 0 ? NS : 1));
  if (cpb > DSEG_CH) cpb = DSEG_CH;
  if (cpb >= 1) {
    // enough workgroups to fill the chip when there are many channels
    while (cpb > 1 && B * ((C + cpb - 1) / cpb) < 512) cpb = (cpb + 1) / 2;
    *cpb_out = cpb;
    *chunk_out = (int)NS;
    return true;
  }
  // several chunks, one channel: a row chunk + the running sum and cursor of every destination
  const int64_t chunk = DSEG_LDS_FLOATS - 2 * R;
  if (chunk < DSEG_MIN_CHUNK) return false;
  *cpb_out = 1;
  *chunk_out = (int)chunk;
  return true;
}

template <bool WEIGHTED>
static int det_segsum(const float* go, int64_t sb, int64_t sc, int64_t s_hi, int64_t s_lo, int64_t inner,
                      const float* weight, int64_t B, int64_t C, int64_t R, int64_t L, const void* plan, float* gi,
                      hipStream_t st) {
  const ScatterPlan pl = scatter_plan_parts(const_cast<void*>(plan), B, R);
  const int64_t NS = WEIGHTED ? L / 3 : L;
  int cpb = 0, chunk = 0;
  if (lds_layout(B, C, R, NS, &cpb, &chunk) && (C + cpb - 1) / cpb <= 65535) {
    static bool attr_set[2] = {false, false};
    if (!attr_set[WEIGHTED]) {
      hipError_t e = hipFuncSetAttribute((const void*)det_segsum_lds_kernel<WEIGHTED>,
                                         hipFuncAttributeMaxDynamicSharedMemorySize, DSEG_LDS_FLOATS * (int)sizeof(float));
      if (e != hipSuccess) return (int)e;
      attr_set[WEIGHTED] = true;
    }
    const bool multi = NS > chunk;
    const size_t lds = sizeof(float) * ((size_t)cpb * chunk + (multi ? (size_t)(cpb + 1) * R : 0));
    const int dense = !WEIGHTED && s_lo == 1 && s_hi == inner;
    dim3 grid((unsigned)((C + cpb - 1) / cpb), (unsigned)B);
    hipLaunchKernelGGL(det_segsum_lds_kernel<WEIGHTED>, grid, dim3(DSEG_T), lds, st, go, sb, sc, s_hi, s_lo, (int)inner,
                       dense, weight, (int)C, (int)R, L, (int)NS, chunk, cpb, pl.off, pl.perm, gi);
    REGNET_LAUNCH_CHECK();
    return REGNET_OK;
  }
  if ((C + DSEG_G_CH - 1) / DSEG_G_CH > 65535 || (R + DSEG_G_T - 1) / DSEG_G_T >= ((int64_t)1 << 31))
    return REGNET_ERR_UNSUPPORTED;
  dim3 grid((unsigned)((R + DSEG_G_T - 1) / DSEG_G_T), (unsigned)((C + DSEG_G_CH - 1) / DSEG_G_CH), (unsigned)B);
  hipLaunchKernelGGL(det_segsum_global_kernel<WEIGHTED>, grid, dim3(DSEG_G_T), 0, st, go, sb, sc, s_hi, s_lo, (int)inner,
                     weight, (int)C, (int)R, L, pl.off, pl.perm, gi);
  REGNET_LAUNCH_CHECK();
  return REGNET_OK;
}

extern "C" int regnet_scatter_segsum_f32(const float* grad_out, int64_t sb, int64_t sc, int64_t s_hi, int64_t s_lo,
                                         int64_t inner, const float* weight, int64_t B, int64_t C, int64_t num_dest,
                                         int64_t num_src, const void* plan, float* grad_in, void* stream) {
  if (B < 0 || C < 0 || num_dest < 0 || num_src < 0 || inner <= 0) return REGNET_ERR_SHAPE;
  if (num_src % inner || (weight && inner != 3)) return REGNET_ERR_SHAPE;
  if (B == 0 || C == 0 || num_dest == 0) return REGNET_OK;
  if (!scatter_plan_dims_ok(B, num_dest, num_src) || inner >= ((int64_t)1 << 31)) return REGNET_ERR_UNSUPPORTED;
  if (!grad_in || !plan) return REGNET_ERR_NULL;
  hipStream_t st = as_stream(stream);
  if (num_src == 0) {
    hipError_t e = hipMemsetAsync(grad_in, 0, sizeof(float) * (size_t)(B * C * num_dest), st);
    return e == hipSuccess ? REGNET_OK : (int)e;
  }
  if (!grad_out) return REGNET_ERR_NULL;
  if (weight) return det_segsum<true>(grad_out, sb, sc, s_hi, 0, 3, weight, B, C, num_dest, num_src, plan, grad_in, st);
  return det_segsum<false>(grad_out, sb, sc, s_hi, s_lo, inner, nullptr, B, C, num_dest, num_src, plan, grad_in, st);
}

// ---- scatter_max_grad --------------------------------------------------------------------------------------------------
// A workgroup per channel f: the R keys (arg[r][f] << 32 | r) are sorted in LDS (bitonic; the keys are distinct, so the
// order is fixed), which lists every destination row's r in ascending order; the thread at the start of a run reads the
// destination once, adds dy[r][f] for the run in order and writes it back.  Rows with arg < 0 sort behind all others and
// add nothing.
#define DSMAX_T 1024
#define DSMAX_ROWS 8192   // keys in LDS: 64 KB

__global__ __launch_bounds__(DSMAX_T) void det_scatter_max_grad_kernel(const float* __restrict__ dy,
                                                                       const int64_t* __restrict__ arg, int R, int F,
                                                                       int Rp, long long scene_rows,
                                                                       long long batch_stride, long long row_stride,
                                                                       long long ch_stride, float* __restrict__ grad) {
  __shared__ unsigned long long key[DSMAX_ROWS];
  const int f = blockIdx.x, t = threadIdx.x;
  for (int r = t; r < Rp; r += DSMAX_T) {
    unsigned long long k = ~0ull;
    if (r < R) {
      const long long row = arg[(int64_t)r * F + f];
      if (row >= 0) k = ((unsigned long long)row << 32) | (unsigned)r;
    }
    key[r] = k;
  }
  for (int size = 2; size <= Rp; size <<= 1) {
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      __syncthreads();
      for (int i = t; i < Rp / 2; i += DSMAX_T) {
        const int lo = 2 * i - (i & (stride - 1)), hi = lo + stride;
        const bool up = (lo & size) == 0;
        const unsigned long long a = key[lo], b = key[hi];
        if ((a > b) == up) { key[lo] = b; key[hi] = a; }
      }
    }
  }
  __syncthreads();
  for (int i = t; i < R; i += DSMAX_T) {
    const unsigned long long k = key[i];
    if (k == ~0ull) continue;
    const long long row = (long long)(k >> 32);
    if (i > 0 && (key[i - 1] >> 32) == (unsigned long long)row) continue;   // not the first of its run
    const long long b = row / scene_rows, n = row - b * scene_rows;
    float* g = grad + b * batch_stride + n * row_stride + (long long)f * ch_stride;
    float v = *g;
    for (int j = i; j < R && key[j] != ~0ull && (long long)(key[j] >> 32) == row; ++j)
      v = v + dy[(int64_t)(unsigned)(key[j] & 0xffffffffu) * F + f];
    *g = v;
  }
}

extern "C" int regnet_scatter_max_grad_det_f32(const float* dy, const int64_t* arg, int64_t R, int64_t F,
                                               int64_t scene_rows, int64_t batch_stride, int64_t row_stride,
                                               int64_t ch_stride, float* grad, void* stream) {
  if (R < 0 || F < 0 || scene_rows <= 0) return REGNET_ERR_SHAPE;
  if (R == 0 || F == 0) return REGNET_OK;
  if (R > DSMAX_ROWS || F > 65535) return REGNET_ERR_UNSUPPORTED;
  if (!dy || !arg || !grad) return REGNET_ERR_NULL;
  int Rp = 2;
  while (Rp < R) Rp <<= 1;
  hipLaunchKernelGGL(det_scatter_max_grad_kernel, dim3((unsigned)F), dim3(DSMAX_T), 0, as_stream(stream), dy, arg, (int)R,
                     (int)F, Rp, (long long)scene_rows, (long long)batch_stride, (long long)row_stride,
                     (long long)ch_stride, grad);
  REGNET_LAUNCH_CHECK();
  return REGNET_OK;
}
