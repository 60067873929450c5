// nms.hip -- pose non-maximum suppression + top-K over one set of grasps on the device (gfx950): the step between the
// network's collision-free grasps and the K distinct ones a robot is handed.
//
// Two grasps are THE SAME GRASP when their centres are close, d2 = ((dx dx) + (dy dy)) + (dz dz) <= T2, and their frames are
// aligned, tr = (da + db) + dm >= C with da / db / dm the dot products of the approach / axis_y / minor-normal columns, each
// ((x x') + (y y')) + (z z'); with `symmetric` the frame turned by 180 degrees about its approach axis counts as well,
// tr2 = (da - db) - dm, and the test is max(tr, tr2) >= C (a NaN on either side fails it).  Built with -ffp-contract=off: every
// product and sum above is individually rounded, in the written order (DESIGN.md par. 3), so a numpy float32 restatement gives
// the same bits.  The grasps arrive ranked (order[r] = input row of rank r, best first); the greedy walk keeps a rank unless an
// already kept one is the same grasp, and stops at top_k.
//
//   * nms_pair_mask_kernel: 64 x 64 tiles over the ranked grasps, upper triangle only.  A wave owns one tile: lane = row, the
//     column block's 12 floats per grasp are staged in LDS and read back as wave-wide broadcasts; one 64-bit word per
//     (row, column block), bit j = "rank cb*64+j is the same grasp as this row", written with ordinary vector stores.
//   * nms_greedy_scan_kernel: ONE workgroup walks the blocks of 64 ranks.  The removed bitmap lives in LDS.  Every wave
//     resolves the block's diagonal word serially in scalar registers (a wave-uniform v_readlane of the kept lane's word per
//     kept rank), then all threads OR the kept rows' words into the removed words of the later blocks.  keep / count are
//     written by plain stores; the walk leaves the loop as soon as top_k ranks are kept.
// No workgroup waits for another: the two launches are ordered by the stream.
#include "common.h"

namespace {

constexpr long long NMS_MAX_N = 32768;
constexpr int NMS_MAX_BLOCKS = (int)(NMS_MAX_N / 64);   // 512 column blocks: one removed word per scan thread & 511
constexpr int NMS_PAIR_WAVES = 4;                        // tiles (column blocks) per pair-mask workgroup
constexpr int NMS_SCAN_THREADS = 1024;
constexpr int NMS_SCAN_UNROLL = 8;                       // kept rows whose words one scan thread has in flight

// The mask is packed by row block: block rb holds 64 rows of (nb - rb) words, the column blocks rb .. nb-1.
__host__ __device__ __forceinline__ long long nms_block_base(long long rb, long long nb) {
  return 64 * (rb * nb - rb * (rb - 1) / 2);
}

// centre (3), approach (3), axis_y (3), minor normal (3) of input row `src`: frame is (n,3,3) with those vectors as COLUMNS
__device__ __forceinline__ void load_pose(const float* __restrict__ center, const float* __restrict__ frame, long long src,
                                          float (&p)[12]) {
  const float* c = center + src * 3;
  const float* f = frame + src * 9;
  p[0] = c[0]; p[1] = c[1]; p[2] = c[2];
  p[3] = f[0]; p[4] = f[3]; p[5] = f[6];
  p[6] = f[1]; p[7] = f[4]; p[8] = f[7];
  p[9] = f[2]; p[10] = f[5]; p[11] = f[8];
}

template <bool SYM>
__global__ __launch_bounds__(NMS_PAIR_WAVES * 64) void nms_pair_mask_kernel(const float* __restrict__ center,
                                                                            const float* __restrict__ frame,
                                                                            const long long* __restrict__ order, int n, int nb,
                                                                            float T2, float C,
                                                                            unsigned long long* __restrict__ mask) {
  __shared__ __attribute__((aligned(16))) float s_col[NMS_PAIR_WAVES][64][12];
  const int rb = blockIdx.y;
  const int cb0 = blockIdx.x * NMS_PAIR_WAVES;
  if (cb0 + NMS_PAIR_WAVES - 1 < rb) return;        // the whole workgroup lies below the diagonal
  const int wave = threadIdx.x >> 6, lane = lane_id();
  const int cb = cb0 + wave;
  const bool active = cb >= rb && cb < nb;
  if (active) {
    // a column past the end, or one whose `order` entry is no row of the input, gets a NaN centre: never close to anything
    float p[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) p[k] = __builtin_nanf("");
    const int j = cb * 64 + lane;
    if (j < n) {
      const long long src = order[j];
      if (src >= 0 && src < n) load_pose(center, frame, src, p);
    }
#pragma unroll
    for (int k = 0; k < 12; ++k) s_col[wave][lane][k] = p[k];
  }
  __syncthreads();
  if (!active) return;

  float r[12];
#pragma unroll
  for (int k = 0; k < 12; ++k) r[k] = __builtin_nanf("");
  const int i = rb * 64 + lane;
  if (i < n) {
    const long long src = order[i];
    if (src >= 0 && src < n) load_pose(center, frame, src, r);
  }
  const float4* col = reinterpret_cast<const float4*>(&s_col[wave][0][0]);
  unsigned long long word = 0;
#pragma unroll 4
  for (int j = 0; j < 64; ++j) {
    const float4 q0 = col[j * 3 + 0], q1 = col[j * 3 + 1], q2 = col[j * 3 + 2];   // c.xyz a.x | a.yz b.xy | b.z m.xyz
    const float d2 = sqdist3(r[0], r[1], r[2], q0.x, q0.y, q0.z);
    const float da = dot3(r[3], r[4], r[5], q0.w, q1.x, q1.y);
    const float db = dot3(r[6], r[7], r[8], q1.z, q1.w, q2.x);
    const float dm = dot3(r[9], r[10], r[11], q2.y, q2.z, q2.w);
    const float tr = (da + db) + dm;
    bool aligned = tr >= C;
    if (SYM) {
      const float tr2 = (da - db) - dm;
      aligned = (aligned || tr2 >= C) && !__builtin_isunordered(tr, tr2);
    }
    const bool same = (d2 <= T2) && aligned;
    word |= (unsigned long long)same << j;
  }
  if (cb == rb) word &= ~((2ull << lane) - 1ull);      // the diagonal tile: only ranks after this row's own
  mask[nms_block_base(rb, nb) + (long long)lane * (nb - rb) + (cb - rb)] = word;   // (rows past n: the padded tail, NaN -> 0)
}

__device__ __forceinline__ unsigned long long readfirstlane64(unsigned long long v) {
  const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)v);
  const unsigned hi = __builtin_amdgcn_readfirstlane((unsigned)(v >> 32));
  return ((unsigned long long)hi << 32) | lo;
}

__device__ __forceinline__ unsigned long long readlane64(unsigned long long v, int lane) {
  const unsigned lo = __builtin_amdgcn_readlane((unsigned)v, lane);
  const unsigned hi = __builtin_amdgcn_readlane((unsigned)(v >> 32), lane);
  return ((unsigned long long)hi << 32) | lo;
}

__global__ __launch_bounds__(NMS_SCAN_THREADS) void nms_greedy_scan_kernel(const unsigned long long* __restrict__ mask,
                                                                           const long long* __restrict__ order, int n, int nb,
                                                                           int top_k, long long* __restrict__ keep,
                                                                           int* __restrict__ count) {
  __shared__ unsigned long long s_removed[NMS_MAX_BLOCKS];
  const int t = threadIdx.x, lane = lane_id();
  const int col = t & (NMS_MAX_BLOCKS - 1);      // the removed word this thread ORs into ...
  const int half = t >> 9;                       // ... for the kept rows 0..31 (threads 0..511) or 32..63 of a block
  if (t < NMS_MAX_BLOCKS) s_removed[t] = 0;
  __syncthreads();
  int total = 0;
  unsigned long long diag = mask[(long long)lane * nb];          // block 0's diagonal words, one row per lane
  for (int rb = 0; rb < nb; ++rb) {
    const long long base = nms_block_base(rb, nb);
    const int width = nb - rb;
    unsigned long long next_diag = 0;
    if (rb + 1 < nb) next_diag = mask[base + 64ll * width + (long long)lane * (width - 1)];   // in flight over this block's work
    const int rows = n - rb * 64;
    const unsigned long long valid = rows >= 64 ? ~0ull : ((1ull << rows) - 1ull);
    // every wave resolves the diagonal for itself, in scalar registers: the ranks still standing, best first
    unsigned long long avail = readfirstlane64(~s_removed[rb] & valid);
    unsigned long long kept = 0;
    const int before = total;
    while (avail != 0 && total < top_k) {
      const int i = __builtin_ctzll(avail);
      kept |= 1ull << i;
      ++total;
      avail &= ~(readlane64(diag, i) | (1ull << i));
    }
    if (t < 64 && ((kept >> lane) & 1ull))
      keep[before + __builtin_popcountll(kept & ((1ull << lane) - 1ull))] = order[rb * 64 + lane];
    if (total >= top_k) break;                   // (uniform over the workgroup: every wave derived the same `kept`)
    unsigned long long mine = half ? (kept & 0xffffffff00000000ull) : (kept & 0xffffffffull);
    if (col > rb && col < nb && mine != 0) {
      const unsigned long long* p = mask + base + (col - rb);
      unsigned long long acc = 0;
      while (mine != 0) {
        unsigned long long v[NMS_SCAN_UNROLL];
#pragma unroll
        for (int u = 0; u < NMS_SCAN_UNROLL; ++u) {
          v[u] = 0;
          if (mine != 0) {
            const int i = __builtin_ctzll(mine);
            mine &= mine - 1ull;
            v[u] = p[(long long)i * width];
          }
        }
#pragma unroll
        for (int u = 0; u < NMS_SCAN_UNROLL; ++u) acc |= v[u];
      }
      if (acc != 0) atomicOr(&s_removed[col], acc);
    }
    __syncthreads();
    diag = next_diag;
  }
  for (int i = total + t; i < n; i += NMS_SCAN_THREADS) keep[i] = -1;
  if (t == 0) *count = total;
}

}  // namespace

extern "C" int64_t regnet_grasp_nms_workspace_bytes(int64_t n) {
  if (n < 0 || n > NMS_MAX_N) return -1;
  const int64_t nb = (n + 63) / 64;
  return nb * (nb + 1) / 2 * 64 * 8;
}

extern "C" int regnet_grasp_nms_f32(const float* center, const float* frame, const int64_t* order, int64_t n, float T2, float C,
                                    int symmetric, int64_t top_k, int64_t* keep, int32_t* count, void* workspace,
                                    void* stream) {
  if (n < 0) return REGNET_ERR_SHAPE;
  if (n == 0) return REGNET_OK;
  if (n > NMS_MAX_N) return REGNET_ERR_UNSUPPORTED;
  if (!center || !frame || !order || !keep || !count || !workspace) return REGNET_ERR_NULL;
  hipStream_t s = as_stream(stream);
  const int nb = (int)((n + 63) / 64);
  const int k = (top_k <= 0 || top_k > n) ? (int)n : (int)top_k;
  unsigned long long* mask = (unsigned long long*)workspace;
  const dim3 grid((unsigned)((nb + NMS_PAIR_WAVES - 1) / NMS_PAIR_WAVES), (unsigned)nb);
  if (symmetric)
    hipLaunchKernelGGL(nms_pair_mask_kernel<true>, grid, dim3(NMS_PAIR_WAVES * 64), 0, s, center, frame,
                       (const long long*)order, (int)n, nb, T2, C, mask);
  else
    hipLaunchKernelGGL(nms_pair_mask_kernel<false>, grid, dim3(NMS_PAIR_WAVES * 64), 0, s, center, frame,
                       (const long long*)order, (int)n, nb, T2, C, mask);
  REGNET_LAUNCH_CHECK();
  hipLaunchKernelGGL(nms_greedy_scan_kernel, dim3(1), dim3(NMS_SCAN_THREADS), 0, s, mask, (const long long*)order, (int)n, nb, k,
                     (long long*)keep, (int*)count);
  REGNET_LAUNCH_CHECK();
  return REGNET_OK;
}
