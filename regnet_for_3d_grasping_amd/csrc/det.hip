// det.hip -- scatter_max_grad of the deterministic mode (torch.use_deterministic_algorithms), gfx950.
//
// The default backward of the pooled region feature (region.hip: scatter_max_grad) adds with float atomics in whatever
// order the hardware runs them.  Here grad[arg[r][f]][f] += dy[r][f] runs in ascending r per channel, onto the value
// already there, so a training iteration gives the same bits run after run.  The mode's segment sums (group /
// gather_knn / interpolate backwards) are in scatter.hip.
//
// Built with -ffp-contract=off (csrc/build.py).
#include "common.h"

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
