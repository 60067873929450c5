// geometry.hip -- furthest point sampling, ball query, 3-NN for gfx950 (CDNA4, wave64).
//
// Built with -ffp-contract=off: every index these kernels emit depends on fp32 compares of
// squared distances, so the arithmetic is pinned to individually rounded IEEE ops (common.h).
//
// Reference behaviour restated (file:line relative to multi_model/utils/pn2_utils/):
//   FPS        csrc/sampling_kernel.cu:47-117
//   ball query csrc/ball_query_kernel.cu:31-74
//   3-NN       csrc/interpolate_kernel.cu:28-77
#include <type_traits>
#include <utility>

#include "common.h"


// =====================================================================================
// Furthest point sampling
// =====================================================================================
// One workgroup per scene; every point's xyz and running min-distance live in VGPRs for
// the whole kernel (PPT points per thread), so a round touches no memory except the
// selected centroid's 12 bytes and one 8-byte LDS slot per wave.
//
// Tie order.  The reference runs `RB = min(2^ceil(log2 N), 512)` threads; thread t scans
// j = t, t+RB, ... keeping its FIRST strict maximum, then a shared-memory tree combines
// lanes with `if (d[t] < d[t+off]) take t+off` for off = RB/2 ... 1.  Among lanes holding the
// global maximum the tree therefore prefers, level by level from the LAST level (off = 1)
// backwards, the lane whose bit is 0: the winner is the lane with the smallest BIT-REVERSED
// lane number, and inside a lane the smallest j.  We reproduce that with a single 64-bit
// max-reduction over  (dist_bits << 32) | ~key,  key = bitrev_log2RB(j mod RB) in the high
// bits and j / RB in the low bits.

__device__ __forceinline__ unsigned fps_key(int j, int rb_log2) {
  unsigned lane = (unsigned)j & ((1u << rb_log2) - 1u);
  return __brev(lane) | ((unsigned)j >> rb_log2);  // __brev puts the reversed lane in the top bits
}
__device__ __forceinline__ int fps_unkey(unsigned key, int rb_log2) {
  unsigned hi_mask = ~(0xffffffffu >> rb_log2);
  unsigned lane = __brev(key & hi_mask);
  return (int)(((key & ~hi_mask) << rb_log2) | lane);
}

__device__ __forceinline__ unsigned long long wave_max_u64(unsigned long long v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    unsigned long long o = __shfl_xor(v, off, 64);
    v = o > v ? o : v;
  }
  return v;
}

// Wave-wide float max without LDS traffic: four DPP steps leave every lane of a 16-lane row with
// the row maximum, the four row results are read back as scalars.
#define DPP_MAX_STEP(v, CTRL)                                                                          \
  v = fmaxf(v, __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(__builtin_bit_cast(int, v),      \
                                                                     __builtin_bit_cast(int, v), CTRL, \
                                                                     0xf, 0xf, false)))
__device__ __forceinline__ float wave_max_f32(float v) {
  DPP_MAX_STEP(v, 0xB1);   // quad_perm [1,0,3,2]
  DPP_MAX_STEP(v, 0x4E);   // quad_perm [2,3,0,1]
  DPP_MAX_STEP(v, 0x141);  // row_half_mirror
  DPP_MAX_STEP(v, 0x140);  // row_mirror
  const int b = __builtin_bit_cast(int, v);
  const float r0 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(b, 0));
  const float r1 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(b, 16));
  const float r2 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(b, 32));
  const float r3 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(b, 48));
  return fmaxf(fmaxf(r0, r1), fmaxf(r2, r3));
}

#define DPP_MINU_STEP(v, CTRL)                                                                                     \
  v = min(v, (unsigned)__builtin_amdgcn_update_dpp((int)v, (int)v, CTRL, 0xf, 0xf, false))
__device__ __forceinline__ unsigned wave_min_u32(unsigned v) {
  DPP_MINU_STEP(v, 0xB1);
  DPP_MINU_STEP(v, 0x4E);
  DPP_MINU_STEP(v, 0x141);
  DPP_MINU_STEP(v, 0x140);
  const unsigned r0 = (unsigned)__builtin_amdgcn_readlane((int)v, 0), r1 = (unsigned)__builtin_amdgcn_readlane((int)v, 16);
  const unsigned r2 = (unsigned)__builtin_amdgcn_readlane((int)v, 32), r3 = (unsigned)__builtin_amdgcn_readlane((int)v, 48);
  return min(min(r0, r1), min(r2, r3));
}
// lexicographic maximum of (hi, lo) pairs over a 16-lane row, left in every lane of the row
#define DPP_MAXPAIR_STEP(hi, lo, CTRL)                                                                             \
  {                                                                                                                \
    const unsigned ohi = (unsigned)__builtin_amdgcn_update_dpp((int)hi, (int)hi, CTRL, 0xf, 0xf, false);           \
    const unsigned olo = (unsigned)__builtin_amdgcn_update_dpp((int)lo, (int)lo, CTRL, 0xf, 0xf, false);           \
    const bool take = ohi > hi || (ohi == hi && olo > lo);                                                         \
    hi = take ? ohi : hi;                                                                                          \
    lo = take ? olo : lo;                                                                                          \
  }


// min(a, b) for non-NaN operands as ONE v_min_f32 (fminf() inserts a canonicalising v_max first).
__device__ __forceinline__ float vmin_f32(float a, float b) {
  float r;
  asm("v_min_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
  return r;
}

// Round structure (2 barriers):
//   scan     every lane: d -> dist = min(dist, d), running thread maximum (VALUE ONLY: 1 v_max/point)
//   stage 1  wave max (DPP) -> LDS -> barrier -> block maximum Mx (wave-uniform)
//   stage 2  only lanes whose maximum equals Mx look up WHICH slot it was and publish the tie-break
//            key with an LDS atomic min -> barrier -> every lane decodes the winner.
// Searching the slot after the fact costs 2 instructions per point in (typically) one wave instead
// of 2 per point in all sixteen.
// ---- sampling a cloud that is itself a furthest-point-sampling sequence (levels 2 and 3 of the network) ----------------
// PointNet++ samples level l+1 from the level-l centroids IN THEIR PICK ORDER, starting from index 0 (pointnet2.py:40-42,
// modules.py:23-26).  Pick k+1 of the level-l run was the point of the WHOLE cloud furthest from picks 0..k; it is one of
// the level-l centroids, so it is also the furthest among THEM, with the same fp32 distance (same two points, same
// formula): the level-(l+1) run re-derives picks 0, 1, 2, ... of level l.  The only way out is a TIE at the maximum,
// which the two runs break by different rules (the reference's tie order depends on positions in the array, and those
// differ).  So a run reports `first_tie` -- the first pick position whose choice was not a unique strict maximum -- and a
// run over its result whose `prefix_ok` (= that value) is >= M writes 0 .. M-1 and returns: no sampling at all, bit-exact
// by construction (and by tests/test_gpu_ops.py against the oracle, which does sample).  Kernels that do not track ties
// report 0 ("unknown"): the next level then samples for real.
__device__ __forceinline__ bool fps_prefix_shortcut(const int* __restrict__ prefix_ok, int* __restrict__ first_tie, int b,
                                                    int M, int64_t* __restrict__ out, int tid, int T, bool writer) {
  if (!prefix_ok) return false;
  const int ok = prefix_ok[b];                    // workgroup-uniform
  if (ok < M) return false;
  if (writer) {
    for (int k = tid; k < M; k += T) out[k] = k;
    if (tid == 0 && first_tie) first_tie[b] = ok;
  }
  return true;
}

template <int T, int PPT>
__global__ __launch_bounds__(T) void fps_resident_kernel(const float* __restrict__ xyz, int64_t sb, int64_t sc,
                                                         int64_t sn, int N, int M, int rb_log2,
                                                         int64_t* __restrict__ index, const int* __restrict__ prefix_ok,
                                                         int* __restrict__ first_tie) {
  constexpr int W = T / 64;
  constexpr int WP = (W + 3) / 4 * 4;
  __shared__ __attribute__((aligned(16))) float part[2][WP];
  __shared__ unsigned win_key[2];
  const int tid = threadIdx.x;
  const float* base = xyz + (int64_t)blockIdx.x * sb;
  int64_t* out = index + (int64_t)blockIdx.x * M;
  if (fps_prefix_shortcut(prefix_ok, first_tie, (int)blockIdx.x, M, out, tid, T, true)) return;
  if (first_tie && tid == 0) first_tie[blockIdx.x] = 0;   // this kernel does not track ties: "unknown"

  float px[PPT], py[PPT], pz[PPT], dist[PPT];
#pragma unroll
  for (int s = 0; s < PPT; ++s) {
    int j = s * T + tid;
    if (j < N) {
      px[s] = base[(int64_t)j * sn];
      py[s] = base[sc + (int64_t)j * sn];
      pz[s] = base[2 * sc + (int64_t)j * sn];
      dist[s] = __builtin_inff();  // "unset" (the reference's -1 with its `last < 0` rule)
    } else {
      px[s] = py[s] = pz[s] = 0.f;
      dist[s] = -1.f;  // padding: min(-1, d) stays -1 and never beats the 0-initialised maximum
    }
  }
  if (tid < 2 * WP) (&part[0][0])[tid] = 0.f;
  if (tid < 2) win_key[tid] = 0xffffffffu;
  if (tid == 0) out[0] = 0;
  __syncthreads();
  int cur = 0;
  for (int i = 1; i < M; ++i) {
    const int buf = i & 1;
    const float cx = base[(int64_t)cur * sn];
    const float cy = base[sc + (int64_t)cur * sn];
    const float cz = base[2 * sc + (int64_t)cur * sn];
    float tmax = 0.f;  // the reference's max_dist = 0 with strict >: only positive distances compete
#pragma unroll
    for (int s = 0; s < PPT; ++s) {
      const float nd = vmin_f32(dist[s], sqdist3(px[s], py[s], pz[s], cx, cy, cz));
      dist[s] = nd;
      tmax = fmaxf(tmax, nd);
    }
    const float wmax = wave_max_f32(tmax);
    if ((tid & 63) == 0) part[buf][tid >> 6] = wmax;
    __syncthreads();
    // Re-arm the slot the NEXT round will use -- only now: it is the slot of the PREVIOUS round, whose winner the other
    // waves read right after that round's last barrier; this barrier is the first point at which all of them have.
    // (Written before the barrier, a wave that ran ahead could wipe the key under a slower wave, which then kept its
    // old centroid: a rare divergence of the waves' `cur`, seen only in the short-scan instantiations under load.)
    if (tid == 0) win_key[buf ^ 1] = 0xffffffffu;
    float mx = 0.f;
#pragma unroll
    for (int w4 = 0; w4 < WP / 4; ++w4) {
      const float4 q = *reinterpret_cast<const float4*>(&part[buf][w4 * 4]);
      mx = fmaxf(fmaxf(mx, fmaxf(q.x, q.y)), fmaxf(q.z, q.w));
    }
    if (mx > 0.f && tmax == mx) {
      int best_s = 0;
#pragma unroll
      for (int s = PPT - 1; s >= 0; --s)
        if (dist[s] == mx) best_s = s;  // first matching slot = smallest j of this reference lane
      atomicMin(&win_key[buf], fps_key(best_s * T + tid, rb_log2));
    }
    __syncthreads();
    const unsigned key = win_key[buf];
    if (key != 0xffffffffu) cur = fps_unkey(key, rb_log2);  // else: every distance is 0 -> repeat cur
    cur = __builtin_amdgcn_readfirstlane(cur);
    if (tid == 0) out[i] = cur;
  }
}

// -------------------------------------------------------------------------------------------
// Large scenes: spatially sorted residency + wave-level skipping.
//
// A new centroid c can lower dist[p] only if |p - c|^2 < dist[p] <= (current maximum of p's
// thread).  If the points a thread holds are spatially compact (bounding sphere (q, R)) the whole
// thread is untouched whenever |q - c| >= R + sqrt(tmax_thread); if that holds for all 64 lanes the
// wave skips the 25-point scan altogether.  Late in the sampling the active radius is a few cm, so
// typically 1-3 of the 16 waves do the scan.  Results are IDENTICAL to the plain kernel: skipped
// updates are provably no-ops (the test is conservative, inflated against fp32 rounding), and the
// arg-max tie-break uses the ORIGINAL point index kept in LDS.
//
// Prologue (once per scene, inside the kernel, no workspace): counting sort of the points by the
// Morton code of a 16x16x16 grid over the scene's bounding box (LDS histogram + scan + scatter of
// the original indices), then thread t loads sorted positions [t*PPT, (t+1)*PPT).
__device__ __forceinline__ unsigned spread4(unsigned v) {  // 4 bits -> every third bit
  return (v & 1u) | ((v & 2u) << 2) | ((v & 4u) << 4) | ((v & 8u) << 6);
}


template <int PPT>
__device__ __forceinline__ float dist_at(const float (&d)[PPT], int s) {  // register array, dynamic index
  float v = d[0];
#pragma unroll
  for (int t = 1; t < PPT; ++t) v = (s == t) ? d[t] : v;
  return v;
}

// max(a, b) / median(a, b, c) for non-NaN operands as ONE instruction each
__device__ __forceinline__ float vmax_f32(float a, float b) {
  float r;
  asm("v_max_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
  return r;
}
__device__ __forceinline__ float vmed3_f32(float a, float b, float c) {
  float r;
  asm("v_med3_f32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
  return r;
}
// maximum over the lane's 16-lane DPP row, left in every lane of the row
__device__ __forceinline__ float row_max_f32(float v) {
  DPP_MAX_STEP(v, 0xB1);
  DPP_MAX_STEP(v, 0x4E);
  DPP_MAX_STEP(v, 0x141);
  DPP_MAX_STEP(v, 0x140);
  return v;
}
__device__ __forceinline__ float readlane_f32(float v, int lane) {
  return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), lane));
}

#ifndef FPS_PICKS
#define FPS_PICKS 4   // picks one round of fps_sorted_kernel may emit (1: the one-pick-per-round loop of rounds 1-2)
#endif

// KP > 1 -- SEVERAL PICKS PER ROUND, exactly.  Furthest point sampling is 5119 DEPENDENT argmax rounds, but the dependence is
// local: the point picked in round i only lowers the running distance of points closer to it than their current value.  If
// the runner-up q2 of round i's argmax is not one of them (|q2 - p1|^2 >= dist[q2]) it keeps its value while nothing else
// can rise, so it IS round i+1's argmax -- provided it beats everything else strictly (ties go to the exact path).  One
// round therefore (1) updates the distances against ALL centroids accepted in the previous round, (2) keeps, per 16-lane row of
// the workgroup (400 spatially compact points), the row's best point and an upper bound v2 on every OTHER point of the row
// (the other lanes' maxima and the owner lane's own second-best), (3) lets wave 0 extract the best rows in order and accept
// candidate j while  v_j > v_(j+1),  v_j > max(v2 of the rows extracted so far)  and  |c_j - a|^2 >= v_j for every centroid a
// accepted before it in this round -- exactly the conditions under which c_j is the unique maximum of the updated field.
// Anything else (equal maxima anywhere near the top, all distances zero) takes the one-pick path with the reference's tie
// order, so the output is bit-identical to the one-pick kernel by construction; on the synthetic scenes 3.7 of 4 candidates are
// accepted per round (5 of 6, 5.9 of 8).  The accepted centroids' coordinates travel through LDS with the candidate
// records: no global load in the round.
template <int PPT, int KP>
__global__ __launch_bounds__(1024) void fps_sorted_kernel(const float* __restrict__ xyz, int64_t sb, int64_t sc,
                                                          int64_t sn, int N, int M, int rb_log2,
                                                          int64_t* __restrict__ index, const int* __restrict__ prefix_ok,
                                                          int* __restrict__ first_tie) {
  constexpr int T = 1024, W = 16, CELLS = 4096;
  if (fps_prefix_shortcut(prefix_ok, first_tie, (int)blockIdx.x, M, index + (int64_t)blockIdx.x * M, (int)threadIdx.x, T, true))
    return;
  if (first_tie && threadIdx.x == 0) first_tie[blockIdx.x] = 0;   // this kernel does not track ties: "unknown"
  __shared__ unsigned perm[T * PPT];   // sorted position -> original index (also the tie-break lookup)
  __shared__ unsigned hist[CELLS];     // histogram, then exclusive offsets
  __shared__ __attribute__((aligned(16))) float part[2][W];
  __shared__ float red[6][W];
  __shared__ unsigned wsum[W];
  __shared__ unsigned win_key[2];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const float* base = xyz + (int64_t)blockIdx.x * sb;
  int64_t* out = index + (int64_t)blockIdx.x * M;

  float px[PPT], py[PPT], pz[PPT], dist[PPT];
  // ---- 1. bounding box of the scene --------------------------------------------------------
  float lo[3] = {__builtin_inff(), __builtin_inff(), __builtin_inff()};
  float hi[3] = {-__builtin_inff(), -__builtin_inff(), -__builtin_inff()};
#pragma unroll
  for (int s = 0; s < PPT; ++s) {
    const int j = s * T + tid;
    if (j < N) {
      px[s] = base[(int64_t)j * sn];
      py[s] = base[sc + (int64_t)j * sn];
      pz[s] = base[2 * sc + (int64_t)j * sn];
      lo[0] = fminf(lo[0], px[s]); hi[0] = fmaxf(hi[0], px[s]);
      lo[1] = fminf(lo[1], py[s]); hi[1] = fmaxf(hi[1], py[s]);
      lo[2] = fminf(lo[2], pz[s]); hi[2] = fmaxf(hi[2], pz[s]);
    } else {
      px[s] = py[s] = pz[s] = 0.f;
    }
  }
#pragma unroll
  for (int a = 0; a < 3; ++a) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      lo[a] = fminf(lo[a], __shfl_xor(lo[a], off, 64));
      hi[a] = fmaxf(hi[a], __shfl_xor(hi[a], off, 64));
    }
    if (lane == 0) { red[a][wave] = lo[a]; red[3 + a][wave] = hi[a]; }
  }
  for (int c = tid; c < CELLS; c += T) hist[c] = 0;
  if (tid < 2 * W) (&part[0][0])[tid] = 0.f;
  if (tid < 2) win_key[tid] = 0xffffffffu;
  if (tid == 0) out[0] = 0;
  __syncthreads();
  float scale[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    float l = red[a][0], h = red[3 + a][0];
#pragma unroll
    for (int w = 1; w < W; ++w) { l = fminf(l, red[a][w]); h = fmaxf(h, red[3 + a][w]); }
    lo[a] = l;
    const float ext = h - l;
    scale[a] = ext > 0.f ? 16.0f / ext : 0.f;
  }
  // ---- 2. counting sort by Morton cell ------------------------------------------------------
  unsigned short cell[PPT], rank[PPT];
#pragma unroll
  for (int s = 0; s < PPT; ++s) {
    const int j = s * T + tid;
    cell[s] = 0; rank[s] = 0;
    if (j < N) {
      const unsigned qx = min(15u, (unsigned)((px[s] - lo[0]) * scale[0]));
      const unsigned qy = min(15u, (unsigned)((py[s] - lo[1]) * scale[1]));
      const unsigned qz = min(15u, (unsigned)((pz[s] - lo[2]) * scale[2]));
      const unsigned c = spread4(qx) | (spread4(qy) << 1) | (spread4(qz) << 2);
      cell[s] = (unsigned short)c;
      rank[s] = (unsigned short)atomicAdd(&hist[c], 1u);
    }
  }
  __syncthreads();
  {  // exclusive scan of hist[4096]: 4 bins per thread, wave scan, scan of the 16 wave sums
    unsigned h0 = hist[4 * tid], h1 = hist[4 * tid + 1], h2 = hist[4 * tid + 2], h3 = hist[4 * tid + 3];
    const unsigned local = h0 + h1 + h2 + h3;
    unsigned incl = local;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const unsigned o = __shfl_up(incl, off, 64);
      if (lane >= off) incl += o;
    }
    if (lane == 63) wsum[wave] = incl;
    __syncthreads();
    unsigned wbase = 0;
#pragma unroll
    for (int w = 0; w < W; ++w) wbase += (w < wave) ? wsum[w] : 0u;
    unsigned o = wbase + incl - local;
    hist[4 * tid] = o; o += h0;
    hist[4 * tid + 1] = o; o += h1;
    hist[4 * tid + 2] = o; o += h2;
    hist[4 * tid + 3] = o;
  }
  __syncthreads();
#pragma unroll
  for (int s = 0; s < PPT; ++s) {
    const int j = s * T + tid;
    if (j < N) perm[hist[cell[s]] + rank[s]] = (unsigned)j;
  }
  __syncthreads();
  // ---- 3. load this thread's spatially consecutive points + bounding sphere -------------------
  float blo[3] = {__builtin_inff(), __builtin_inff(), __builtin_inff()};
  float bhi[3] = {-__builtin_inff(), -__builtin_inff(), -__builtin_inff()};
#pragma unroll
  for (int s = 0; s < PPT; ++s) {
    const int q = tid * PPT + s;
    if (q < N) {
      const int64_t j = perm[q];
      px[s] = base[j * sn];
      py[s] = base[sc + j * sn];
      pz[s] = base[2 * sc + j * sn];
      dist[s] = __builtin_inff();
      blo[0] = fminf(blo[0], px[s]); bhi[0] = fmaxf(bhi[0], px[s]);
      blo[1] = fminf(blo[1], py[s]); bhi[1] = fmaxf(bhi[1], py[s]);
      blo[2] = fminf(blo[2], pz[s]); bhi[2] = fmaxf(bhi[2], pz[s]);
    } else {
      px[s] = py[s] = pz[s] = 0.f;
      dist[s] = -1.f;
    }
  }
  const bool has_points = tid * PPT < N;
  const float qx = has_points ? 0.5f * (blo[0] + bhi[0]) : 0.f;
  const float qy = has_points ? 0.5f * (blo[1] + bhi[1]) : 0.f;
  const float qz = has_points ? 0.5f * (blo[2] + bhi[2]) : 0.f;
  float r2 = 0.f;
#pragma unroll
  for (int s = 0; s < PPT; ++s)
    if (tid * PPT + s < N) r2 = fmaxf(r2, sqdist3(px[s], py[s], pz[s], qx, qy, qz));
  const float R = sqrtf(r2) * 1.0001f + 1e-12f;         // conservative cluster radius
  float tmax = 0.f;
  float thr = has_points ? __builtin_inff() : -1.f;      // update needed while |q - c|^2 < thr

  if constexpr (KP > 1) {
    __shared__ float4 rrec_a[64];      // per row: (best value, bound on every other point of the row, best point's x, y)
    __shared__ float2 rrec_b[64];      //          (z, sorted position of the best point)
    __shared__ float4 accb[KP];        // centroids accepted in the last round: (x, y, z, original index)
    __shared__ int acc_n;              // how many; 0 = "take the exact one-pick path"
    __shared__ float fb_mx;            // the block maximum, for that path
    if (tid == 0) {
      accb[0] = make_float4(base[0], base[sc], base[2 * sc], __int_as_float(0));
      acc_n = 1;
    }
    if (tid < 64) {
      rrec_a[tid] = make_float4(-1.f, -1.f, 0.f, 0.f);
      rrec_b[tid] = make_float2(0.f, 0.f);
    }
    __syncthreads();
    int i = 1, last = 0;
    while (i < M) {
      const int n = __builtin_amdgcn_readfirstlane(acc_n);
      bool scanned = false;
      for (int c = 0; c < n; ++c) {
        const float4 a = accb[c];
        const float cx = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, a.x)));
        const float cy = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, a.y)));
        const float cz = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, a.z)));
        const bool need = sqdist3(qx, qy, qz, cx, cy, cz) < thr;
        if (__ballot(need) != 0ull) {
#pragma unroll
          for (int s = 0; s < PPT; ++s) dist[s] = vmin_f32(dist[s], sqdist3(px[s], py[s], pz[s], cx, cy, cz));
          scanned = true;
        }
      }
      if (scanned) {   // wave-uniform: this wave's rows get new records
        float t1 = dist[0], t2 = -1.f;
#pragma unroll
        for (int s = 1; s < PPT; ++s) {
          t2 = vmed3_f32(t1, t2, dist[s]);      // second largest so far (t1 >= t2)
          t1 = vmax_f32(t1, dist[s]);
        }
        tmax = t1;
        const float reach = R + sqrtf(fmaxf(t1, 0.f)) * 1.0001f;
        thr = has_points ? reach * reach * 1.0001f + 1e-30f : -1.f;
        float sx = px[0], sy = py[0], sz = pz[0];
        int slot = 0;
#pragma unroll
        for (int s = 1; s < PPT; ++s) {
          const bool hit = dist[s] == t1;
          sx = hit ? px[s] : sx;
          sy = hit ? py[s] : sy;
          sz = hit ? pz[s] : sz;
          slot = hit ? s : slot;
        }
        const float rmax = row_max_f32(t1);
        const bool hit = t1 == rmax;
        const unsigned seg = (unsigned)(__ballot(hit) >> (lane & 48)) & 0xffffu;
        const bool owner = hit && (seg & ((1u << (lane & 15)) - 1u)) == 0u;     // the row's first lane holding its maximum
        const float r2 = row_max_f32(owner ? t2 : t1);    // everything in the row but the owner's best point
        if (owner) {
          const int row = wave * 4 + (lane >> 4);
          rrec_a[row] = make_float4(rmax, r2, sx, sy);
          rrec_b[row] = make_float2(sz, __int_as_float(tid * PPT + slot));
        }
      }
      __syncthreads();
      if (wave == 0) {
        const float4 ra = rrec_a[lane];
        const float2 rb = rrec_b[lane];
        float v = ra.x;
        const float m0 = wave_max_f32(v);
        unsigned long long mk = __ballot(v == m0);
        int lj = __builtin_amdgcn_readfirstlane(__ffsll((long long)mk) - 1);
        float bmax = readlane_f32(ra.y, lj);
        bool ok = m0 > 0.f && __popcll(mk) == 1 && m0 > bmax;
        v = lane == lj ? -2.f : v;
        float mnext = wave_max_f32(v);
        ok = ok && m0 > mnext;
        int cnt = 0;
        float ax = 0.f, ay = 0.f, az = 0.f;
        int aq = 0;                      // lane t < cnt: the t-th centroid accepted in this round
        if (ok) {
          float mj = m0;
          for (;;) {
            const float cjx = readlane_f32(ra.z, lj), cjy = readlane_f32(ra.w, lj), cjz = readlane_f32(rb.x, lj);
            const int cq = __builtin_amdgcn_readlane(__float_as_int(rb.y), lj);
            if (cnt > 0) {               // is the candidate untouched by the centroids accepted before it?
              const float d = sqdist3(cjx, cjy, cjz, ax, ay, az);
              if (__ballot(lane < cnt && d < mj) != 0ull) break;
            }
            if (lane == cnt) { ax = cjx; ay = cjy; az = cjz; aq = cq; }
            ++cnt;
            if (cnt == KP || i + cnt >= M) break;
            mj = mnext;
            if (!(mj > 0.f)) break;
            mk = __ballot(v == mj);
            if (__popcll(mk) != 1) break;
            lj = __builtin_amdgcn_readfirstlane(__ffsll((long long)mk) - 1);
            bmax = fmaxf(bmax, readlane_f32(ra.y, lj));
            v = lane == lj ? -2.f : v;
            mnext = wave_max_f32(v);
            if (!(mj > mnext && mj > bmax)) break;
          }
        }
        if (lane < cnt) {
          const int idx = (int)perm[aq];
          accb[lane] = make_float4(ax, ay, az, __int_as_float(idx));
          out[i + lane] = idx;
        }
        if (lane == 0) { acc_n = cnt; fb_mx = m0; }
      }
      __syncthreads();
      const int got = __builtin_amdgcn_readfirstlane(acc_n);
      if (got > 0) {
        last = __builtin_amdgcn_readfirstlane(__float_as_int(accb[got - 1].w));
        i += got;
        continue;
      }
      // ---- exact one-pick path (equal maxima / all distances zero): the reference's tie order through the keys ----------
      const float mx = fb_mx;
      if (mx > 0.f && tmax == mx) {
        unsigned kmin = 0xffffffffu;
#pragma unroll     // (static slots: a rolled loop would make the compiler keep a scratch copy of dist[] alive in the hot loop)
        for (int s = 0; s < PPT; ++s)
          if (dist[s] == mx) kmin = min(kmin, fps_key((int)perm[tid * PPT + s], rb_log2));
        atomicMin(&win_key[0], kmin);
      }
      __syncthreads();
      const unsigned key = win_key[0];
      const int cur1 = key != 0xffffffffu ? fps_unkey(key, rb_log2) : last;   // all distances 0: the reference repeats cur
      __syncthreads();
      if (tid == 0) {
        win_key[0] = 0xffffffffu;
        accb[0] = make_float4(base[(int64_t)cur1 * sn], base[sc + (int64_t)cur1 * sn], base[2 * sc + (int64_t)cur1 * sn],
                              __int_as_float(cur1));
        acc_n = 1;
        out[i] = cur1;
      }
      last = cur1;
      i += 1;
      __syncthreads();
    }
    return;
  }

  int cur = 0;
  for (int i = 1; i < M; ++i) {
    const int buf = i & 1;
    const float cx = base[(int64_t)cur * sn];
    const float cy = base[sc + (int64_t)cur * sn];
    const float cz = base[2 * sc + (int64_t)cur * sn];
    const bool need = sqdist3(qx, qy, qz, cx, cy, cz) < thr;
    if (__ballot(need) != 0ull) {  // wave-uniform: scan all 64 lanes' points (extra updates are no-ops)
      float m = 0.f;
#pragma unroll
      for (int s = 0; s < PPT; ++s) {
        const float nd = vmin_f32(dist[s], sqdist3(px[s], py[s], pz[s], cx, cy, cz));
        dist[s] = nd;
        m = fmaxf(m, nd);
      }
      tmax = m;
      const float reach = R + sqrtf(m) * 1.0001f;
      thr = has_points ? reach * reach * 1.0001f + 1e-30f : -1.f;
    }
    const float wmax = wave_max_f32(tmax);
    if (lane == 0) part[buf][wave] = wmax;
    __syncthreads();
    if (tid == 0) win_key[buf ^ 1] = 0xffffffffu;   // after the barrier: see fps_resident_kernel
    float mx = 0.f;
#pragma unroll
    for (int w4 = 0; w4 < W / 4; ++w4) {
      const float4 v = *reinterpret_cast<const float4*>(&part[buf][w4 * 4]);
      mx = fmaxf(fmaxf(mx, fmaxf(v.x, v.y)), fmaxf(v.z, v.w));
    }
    if (mx > 0.f && tmax == mx) {
      // which slot(s) hold the maximum?  Branch-free count + last match (pure VALU), ONE LDS read
      // for the usual single match; several equal maxima in one thread (duplicated points) take
      // the slow path that compares every matching slot's tie-break key.
      int nmatch = 0, slot = 0;
#pragma unroll
      for (int s = 0; s < PPT; ++s) {
        const bool hit = dist[s] == mx;
        nmatch += hit ? 1 : 0;
        slot = hit ? s : slot;
      }
      unsigned kmin = fps_key((int)perm[tid * PPT + slot], rb_log2);
      if (nmatch > 1) {
#pragma unroll 1
        for (int s = 0; s < PPT; ++s)
          if (dist_at(dist, s) == mx) kmin = min(kmin, fps_key((int)perm[tid * PPT + s], rb_log2));
      }
      atomicMin(&win_key[buf], kmin);
    }
    __syncthreads();
    const unsigned key = win_key[buf];
    if (key != 0xffffffffu) cur = fps_unkey(key, rb_log2);
    cur = __builtin_amdgcn_readfirstlane(cur);
    if (tid == 0) out[i] = cur;
  }
}

// ---- cluster layout -----------------------------------------------------------------------------------------------------
// fps_sorted_kernel prunes per WAVE: a wave whose 1600 spatially compact points might be touched by a centroid updates all 25
// of its slots (225 instructions), although the centroid changes a handful of points -- and with several centroids per round
// the workgroup is bound by the VALU issue rate of its one CU (~9 800 wave-instructions per round at 8 candidates, 64 % of them
// such scans; scripts/ablate/fps_ablate.cpp).  Here the pruning unit is what the hardware executes as a unit: ONE slot of ONE
// wave = a CLUSTER of 64 consecutive points of the Morton order (cluster g lives in slot g / 16 of wave g % 16: neighbouring
// clusters sit in different waves).  Lane s of a wave keeps the bounding sphere and the current maximum of the wave's cluster
// s, so one vector comparison tests a centroid against all 25 clusters of the wave; a flagged cluster costs 9 instructions for
// the distances plus two wave reductions for its record (best value, bound on the rest, the best point's coordinates straight
// from the slot's registers -- no search), and ~11 of the 400 clusters are flagged per centroid.  Wave 0 folds the 400 records
// into 64 lane records and runs the ordered acceptance of fps_sorted_kernel<.., KP> on them.  Same picks, bit for bit.
__device__ __forceinline__ float wave_min_f32(float v) { return -wave_max_f32(-v); }

// wave maximum of non-NaN values with one instruction per DPP step (fmaxf() costs a canonicalising v_max and two moves per
// step); the s_nop covers the VALU-write -> DPP-read hazard the assembler does not see inside inline asm
__device__ __forceinline__ float wave_max_fast(float v) {
  asm("s_nop 1\n\tv_max_f32_dpp %0, %0, %0 quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf\n\t"
      "s_nop 1\n\tv_max_f32_dpp %0, %0, %0 quad_perm:[2,3,0,1] row_mask:0xf bank_mask:0xf\n\t"
      "s_nop 1\n\tv_max_f32_dpp %0, %0, %0 row_half_mirror row_mask:0xf bank_mask:0xf\n\t"
      "s_nop 1\n\tv_max_f32_dpp %0, %0, %0 row_mirror row_mask:0xf bank_mask:0xf\n\ts_nop 1"
      : "+v"(v));
  const int b = __builtin_bit_cast(int, v);
  const float r0 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(b, 0));
  const float r1 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(b, 16));
  const float r2 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(b, 32));
  const float r3 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(b, 48));
  return vmax_f32(vmax_f32(r0, r1), vmax_f32(r2, r3));
}

template <int PPT>
__device__ __forceinline__ void fps_morton_perm(const float* __restrict__ base, int64_t sc, int64_t sn, int N, unsigned* perm,
                                                unsigned* hist, float (*red)[16], unsigned* wsum) {
  // counting sort of the points by the Morton code of a 16^3 grid over the bounding box: perm[sorted position] = original index
  constexpr int T = 1024, W = 16, CELLS = 4096;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  float lo[3] = {__builtin_inff(), __builtin_inff(), __builtin_inff()};
  float hi[3] = {-__builtin_inff(), -__builtin_inff(), -__builtin_inff()};
  float px[PPT], py[PPT], pz[PPT];
#pragma unroll
  for (int s = 0; s < PPT; ++s) {
    const int j = s * T + tid;
    px[s] = py[s] = pz[s] = 0.f;
    if (j < N) {
      px[s] = base[(int64_t)j * sn];
      py[s] = base[sc + (int64_t)j * sn];
      pz[s] = base[2 * sc + (int64_t)j * sn];
      lo[0] = fminf(lo[0], px[s]); hi[0] = fmaxf(hi[0], px[s]);
      lo[1] = fminf(lo[1], py[s]); hi[1] = fmaxf(hi[1], py[s]);
      lo[2] = fminf(lo[2], pz[s]); hi[2] = fmaxf(hi[2], pz[s]);
    }
  }
#pragma unroll
  for (int a = 0; a < 3; ++a) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      lo[a] = fminf(lo[a], __shfl_xor(lo[a], off, 64));
      hi[a] = fmaxf(hi[a], __shfl_xor(hi[a], off, 64));
    }
    if (lane == 0) { red[a][wave] = lo[a]; red[3 + a][wave] = hi[a]; }
  }
  for (int c = tid; c < CELLS; c += T) hist[c] = 0;
  __syncthreads();
  // 12 key bits, dealt one at a time to the axis whose cells are currently the longest: the cells come out as close to cubes
  // as 4096 of them can be (a table-top scene is a slab: 16 x 16 x 16 would spend a third of the bits on a few centimetres of
  // depth and leave flat, wide cells -- and clusters three times the radius).  Bits are interleaved in the order dealt.
  float scale[3], ext[3];
  int nb[3] = {0, 0, 0};
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    float l = red[a][0], h = red[3 + a][0];
#pragma unroll
    for (int w = 1; w < W; ++w) { l = fminf(l, red[a][w]); h = fmaxf(h, red[3 + a][w]); }
    lo[a] = l;
    ext[a] = h - l;
  }
  unsigned order = 0;   // 2 bits per key bit, most significant key bit first: which axis it came from
#pragma unroll
  for (int k = 0; k < 12; ++k) {
    const float e0 = ext[0] / (float)(1 << nb[0]), e1 = ext[1] / (float)(1 << nb[1]), e2 = ext[2] / (float)(1 << nb[2]);
    const int a = (e0 >= e1 && e0 >= e2) ? 0 : (e1 >= e2 ? 1 : 2);
    nb[a] += 1;
    order = (order << 2) | (unsigned)a;
  }
#pragma unroll
  for (int a = 0; a < 3; ++a) scale[a] = ext[a] > 0.f ? (float)(1 << nb[a]) / ext[a] : 0.f;
  unsigned short cell[PPT], rank[PPT];
#pragma unroll
  for (int s = 0; s < PPT; ++s) {
    const int j = s * T + tid;
    cell[s] = 0; rank[s] = 0;
    if (j < N) {
      unsigned q[3];
      q[0] = min((1u << nb[0]) - 1u, (unsigned)((px[s] - lo[0]) * scale[0]));
      q[1] = min((1u << nb[1]) - 1u, (unsigned)((py[s] - lo[1]) * scale[1]));
      q[2] = min((1u << nb[2]) - 1u, (unsigned)((pz[s] - lo[2]) * scale[2]));
      int left[3] = {nb[0], nb[1], nb[2]};
      unsigned c = 0;
#pragma unroll
      for (int k = 11; k >= 0; --k) {
        const int a = (order >> (2 * k)) & 3;
        left[a] -= 1;
        c = (c << 1) | ((q[a] >> left[a]) & 1u);
      }
      cell[s] = (unsigned short)c;
      rank[s] = (unsigned short)atomicAdd(&hist[c], 1u);
    }
  }
  __syncthreads();
  {
    unsigned h0 = hist[4 * tid], h1 = hist[4 * tid + 1], h2 = hist[4 * tid + 2], h3 = hist[4 * tid + 3];
    const unsigned local = h0 + h1 + h2 + h3;
    unsigned incl = local;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const unsigned o = __shfl_up(incl, off, 64);
      if (lane >= off) incl += o;
    }
    if (lane == 63) wsum[wave] = incl;
    __syncthreads();
    unsigned wbase = 0;
#pragma unroll
    for (int w = 0; w < W; ++w) wbase += (w < wave) ? wsum[w] : 0u;
    unsigned o = wbase + incl - local;
    hist[4 * tid] = o; o += h0;
    hist[4 * tid + 1] = o; o += h1;
    hist[4 * tid + 2] = o; o += h2;
    hist[4 * tid + 3] = o;
  }
  __syncthreads();
#pragma unroll
  for (int s = 0; s < PPT; ++s) {
    const int j = s * T + tid;
    if (j < N) perm[hist[cell[s]] + rank[s]] = (unsigned)j;
  }
  __threadfence_block();   // perm may live in global memory (read back by other waves of this workgroup)
  __syncthreads();
}

// The per-slot state is 25 x 4 NAMED scalars, not arrays: with arrays the compiler sinks the identical stores of the 25 switch
// cases into one indexed store, turns the arrays into 16-/25-register tuples and spills them (700 spill instructions).
#define FPS_SLOTS(X) X(0) X(1) X(2) X(3) X(4) X(5) X(6) X(7) X(8) X(9) X(10) X(11) X(12) X(13) X(14) X(15) X(16) X(17) X(18) \
  X(19) X(20) X(21) X(22) X(23) X(24)
#define FPS_SLOT_DECL(S) float px##S = 0.f, py##S = 0.f, dist##S = -1.f;   // z lives in LDS (pzl): 128 registers per lane
// load slot S (sorted position (S * 16 + wave) * 64 + lane) and give lane S the bounding sphere of the wave's cluster S
#define FPS_SLOT_LOAD(S)                                                                                               \
  if constexpr (S < PPT) {                                                                                             \
    const int q = (S * 16 + wave) * 64 + lane;                                                                         \
    const bool valid = q < Nl;                                                                                         \
    float pz_ = 0.f;                                                                                                   \
    if (valid) {                                                                                                       \
      const int64_t j = perm[q];                                                                                       \
      px##S = lbase[j * sn];                                                                                           \
      py##S = lbase[sc + j * sn];                                                                                      \
      pz_ = lbase[2 * sc + j * sn];                                                                                    \
      dist##S = __builtin_inff();                                                                                      \
    }                                                                                                                  \
    pzl[q] = pz_;                                                                                                      \
    const float inf = __builtin_inff();                                                                                \
    const float lx = wave_min_f32(valid ? px##S : inf), hx = wave_max_f32(valid ? px##S : -inf);                       \
    const float ly = wave_min_f32(valid ? py##S : inf), hy = wave_max_f32(valid ? py##S : -inf);                       \
    const float lz = wave_min_f32(valid ? pz_ : inf), hz = wave_max_f32(valid ? pz_ : -inf);                           \
    const bool any = __ballot(valid) != 0ull;                                                                          \
    const float mx_ = 0.5f * (lx + hx), my_ = 0.5f * (ly + hy), mz_ = 0.5f * (lz + hz);                                \
    const float r2 = wave_max_f32(valid ? sqdist3(px##S, py##S, pz_, mx_, my_, mz_) : 0.f);                            \
    if (lane == S && any) {                                                                                            \
      cqx = mx_; cqy = my_; cqz = mz_;                                                                                 \
      cR = sqrtf(r2) * 1.0001f + 1e-12f; /* conservative cluster radius */                                             \
      cthr = __builtin_inff();           /* update needed while |q - c|^2 < cthr */                                    \
    }                                                                                                                  \
  }
#define FPS_CLUSTER_MAX_PICKS 8192   // picks of one launch kept in LDS (32 KB); longer runs take fps_sorted_kernel
// one flagged cluster: distances, then (if any changed) the cluster's record and its maximum for the sphere test
#define FPS_CLUSTER_UPDATE(S)                                                                                          \
  case S:                                                                                                              \
    if constexpr (S < PPT) {                                                                                           \
      const float od = dist##S;                                                                                        \
      float cx_ = cx, cy_ = cy, cz_ = cz; /* opaque: or all 25 slots' distances are hoisted in front of the switch, */  \
      int t_ = tid;                       /* and 25 x 3 loop-invariant addresses / values live in registers         */  \
      asm volatile("" : "+v"(cx_), "+v"(cy_), "+v"(cz_), "+v"(t_));                                                    \
      const float pz_ = pzl[S * 1024 + t_];                                                                            \
      const float nd = vmin_f32(od, sqdist3(px##S, py##S, pz_, cx_, cy_, cz_));                                        \
      dist##S = nd;                                                                                                    \
      if (__ballot(nd < od) != 0ull) {                                                                                 \
        const float m = wave_max_fast(nd);                                                                             \
        const int own = __builtin_amdgcn_readfirstlane(__ffsll((long long)__ballot(nd == m)) - 1);                     \
        const float m2 = wave_max_fast(lane == own ? -1.f : nd);                                                       \
        if (lane == own) {                                                                                             \
          rec_v[S * 16 + (t_ >> 6)] = make_float2(m, m2);                                                              \
          rec_p[S * 16 + (t_ >> 6)] = make_float4(px##S, py##S, pz_, __int_as_float(S * 1024 + t_));                   \
        }                                                                                                              \
        cmax = lane == S ? m : cmax;                                                                                   \
        touched = true;                                                                                                \
      }                                                                                                                \
    }                                                                                                                  \
    break;
#define FPS_SLOT_FALLBACK(S)                                                                                           \
  if constexpr (S < PPT) {                                                                                             \
    if (dist##S == mx) { kmin = min(kmin, fps_key(n0 + (int)perm[S * 1024 + tid], rb_log2)); nm += 1; }                \
  }

// MULTI: G = 2..4 cooperating workgroups per scene (scenes beyond one CU's registers: 25 600 < N <= 102 400).  Workgroup h owns
// the slice [h Nh, (h + 1) Nh) of the scene -- its own Morton sort, clusters and records -- and the selection is REPLICATED: per
// round every workgroup publishes its 64 lane records (2 KB) to global memory behind a round tag, reads the others', merges them
// in workgroup order and runs the same acceptance on the same values, so all of them accept the same centroids without a second
// exchange.  One exchange per ROUND (~6 picks) where fps_multi_kernel pays one per pick.  The exact one-pick path exchanges
// the workgroups' smallest tie-break keys the same way.  Every workgroup of a scene must be resident (the launcher checks
// G x B against the CU count; a poll gives up after 2^22 tries instead of hanging the device).
#define FPS_XCHG_FLOATS (2 * 4 * 64 * 8)             // [parity][workgroup][lane][8] per scene
#define FPS_XCHG_BYTES (FPS_XCHG_FLOATS * 4 + 256)   // + round tags [4] and key words [parity][4]
#define FPS_STATUS_BYTES 256                         // behind the B scenes' areas: ONE status word per launch (bit 0: a poll's
                                                     // budget ran out -- a partner workgroup was not resident / lost)
#define FPS_LOST_KEY 0xfffffffeu                     // win_key value that ends the round loop (no point has this key)
template <int PPT, int KP, bool MULTI>
__global__ __launch_bounds__(1024) void fps_cluster_kernel(const float* __restrict__ xyz, int64_t sb, int64_t sc,
                                                           int64_t sn, int N, int M, int rb_log2,
                                                           unsigned* __restrict__ perm_ws, int64_t* __restrict__ index,
                                                           int G, int B, int Bpad, float* __restrict__ xchg_ws,
                                                           const int* __restrict__ prefix_ok, int* __restrict__ first_tie) {
  static_assert(PPT <= 25 && KP >= 1 && KP <= 15, "one lane per cluster of a wave, one DPP row of candidates");
  constexpr int T = 1024, W = 16, CELLS = 4096, C = PPT * 16;
  __shared__ float pzl[T * PPT];     // z of sorted position q (x, y and the running distance are registers)
  unsigned* hist = reinterpret_cast<unsigned*>(pzl);   // the sort's histogram: dead before pzl is filled
  static_assert(T * PPT >= CELLS, "histogram aliases pzl");
  int b = (int)blockIdx.x, h = 0;
  if constexpr (MULTI) {
    b = (int)(blockIdx.x % (unsigned)Bpad);           // a scene's workgroups: blockIdx b + h Bpad (one XCD when Bpad % 8 == 0)
    h = (int)(blockIdx.x / (unsigned)Bpad);
    if (b >= B) return;
  }
  if (fps_prefix_shortcut(prefix_ok, first_tie, b, M, index + (int64_t)b * M, (int)threadIdx.x, 1024, h == 0)) return;
  const int Nh = MULTI ? (N + G - 1) / G : N;          // slice length; this workgroup's slice is [n0, n0 + Nl)
  const int n0 = h * Nh, Nl = min(N - n0, Nh);
  unsigned* perm = perm_ws + (int64_t)b * N + n0;      // sorted position -> index inside the slice: N words of workspace per scene
  __shared__ float red[6][W];
  __shared__ unsigned wsum[W];
  __shared__ unsigned win_key;
  constexpr int CP = (C + 63) / 64 * 64;
  __shared__ float2 rec_v[CP];       // per cluster: (best value, bound on its other points); padded with -1 to whole waves
  __shared__ float4 rec_p[C];        //              the best point's (x, y, z, sorted position)
  __shared__ float4 accb[KP];
  __shared__ int acc_n;
  __shared__ float fb_mx;
  __shared__ int picks[FPS_CLUSTER_MAX_PICKS];   // M <= FPS_CLUSTER_MAX_PICKS (the launcher checks)
  __shared__ float4 cand_p[16];      // wave 0's selection: the surviving candidates (x, y, z, value) ...
  __shared__ int cand_q[16];         // ... their sorted positions ...
  __shared__ int rank_buf[64];       // ... and the partial ranks of the pairwise pass
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const float* base = xyz + (int64_t)b * sb;
  const float* lbase = base + (int64_t)n0 * sn;
  int64_t* out = index + (int64_t)b * M;
  float* const xch = MULTI ? xchg_ws + (int64_t)b * (FPS_XCHG_BYTES / 4) : nullptr;
  unsigned* const tags = reinterpret_cast<unsigned*>(xch + FPS_XCHG_FLOATS);                            // [4]
  unsigned long long* const keyw = reinterpret_cast<unsigned long long*>(xch + FPS_XCHG_FLOATS + 16);   // [2 parities][4]
  unsigned* const status = MULTI ? reinterpret_cast<unsigned*>(xchg_ws + (int64_t)B * (FPS_XCHG_BYTES / 4)) : nullptr;
  fps_morton_perm<PPT>(lbase, sc, sn, Nl, perm, hist, red, wsum);

  FPS_SLOTS(FPS_SLOT_DECL)
  float cqx = 0.f, cqy = 0.f, cqz = 0.f, cR = 0.f, cthr = -1.f, cmax = __builtin_inff();   // lane s: cluster s * 16 + wave
  FPS_SLOTS(FPS_SLOT_LOAD)
  for (int g = tid; g < CP; g += T) {
    rec_v[g] = make_float2(-1.f, -1.f);
    if (g < C) rec_p[g] = make_float4(0.f, 0.f, 0.f, 0.f);
  }
  __shared__ int tie_cnt;                     // one-pick path: points holding the maximum (this workgroup's)
  if (tid == 0) {
    accb[0] = make_float4(base[0], base[sc], base[2 * sc], __int_as_float(-1));
    acc_n = 1;
    win_key = 0xffffffffu;
    tie_cnt = 0;
    picks[0] = -1;                            // entries < 0: -(original index + 1); >= 0: workgroup << 24 | sorted position
  }
  __syncthreads();
  int tie_at = 0x7fffffff;                    // (thread 0) first pick position that was not a unique strict maximum
  int i = 1;
  unsigned round = 0;                         // MULTI: exchange tag (every workgroup of the scene runs the same rounds)
  float rho = 0.5f;                           // wave 0: candidate threshold as a fraction of the maximum (adaptive)
  while (i < M) {
    const int n = __builtin_amdgcn_readfirstlane(acc_n);
    bool touched = false;
    for (int c = 0; c < n; ++c) {
      const float4 a = accb[c];
      const float cx = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, a.x)));
      const float cy = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, a.y)));
      const float cz = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, a.z)));
      unsigned mask = (unsigned)__ballot(sqdist3(cqx, cqy, cqz, cx, cy, cz) < cthr);    // lanes >= PPT: cthr = -1
      while (mask) {
        const int s = __builtin_ctz(mask);
        mask &= mask - 1;
        switch (s) {
          FPS_SLOTS(FPS_CLUSTER_UPDATE)
          default: break;
        }
      }
    }
    if (touched) {
      const float reach = cR + sqrtf(fmaxf(cmax, 0.f)) * 1.0001f;
      cthr = cthr >= 0.f ? reach * reach * 1.0001f + 1e-30f : -1.f;
    }
    __syncthreads();
    if (wave == 0) {
      // 64 lane records out of the C cluster records: the lane's best cluster and a bound on everything else it looked at
      int l_ = lane;                       // opaque: addresses derived from it are recomputed here, not kept (spilled) across the loop
      asm volatile("" : "+v"(l_));
      float v = -1.f, v2 = -1.f, y1 = -1.f;
      int gb = l_;
      float2 rr[CP / 64];
#pragma unroll
      for (int k = 0; k < CP / 64; ++k) rr[k] = rec_v[k * 64 + l_];      // all loads in flight together (no guards: padded)
#pragma unroll
      for (int k = 0; k < CP / 64; ++k) {
        const bool better = rr[k].x > v;
        v2 = vmax_f32(v2, better ? v : rr[k].x);
        y1 = better ? rr[k].y : y1;
        gb = better ? k * 64 + l_ : gb;
        v = better ? rr[k].x : v;
      }
      v2 = vmax_f32(v2, y1);
      float4 rp = rec_p[gb];
      rp.w = __int_as_float((h << 24) | __float_as_int(rp.w));     // pick code: workgroup << 24 | sorted position
      bool lost = false;
      if constexpr (MULTI) {
        // publish this workgroup's 64 lane records, fetch the others', merge in workgroup order (identical in every workgroup)
        round += 1;
        float* const slot0 = xch + ((round & 1u) * 4u) * 512u;
        float* const mine = slot0 + h * 512 + l_ * 8;
        reinterpret_cast<float4*>(mine)[0] = make_float4(v, v2, rp.x, rp.y);
        reinterpret_cast<float4*>(mine)[1] = make_float4(rp.z, rp.w, 0.f, 0.f);
        __threadfence();                                            // the records before the tag
        if (l_ == 0) __hip_atomic_store(&tags[h], round, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
        float bv = -3.f, bv2 = -3.f, rest = -3.f;
        float4 brp = rp;
        for (int o = 0; o < G; ++o) {
          float ov = v, ov2 = v2;
          float4 orp = rp;
          if (o != h) {
            int budget = 1 << 22;
            while (__hip_atomic_load(&tags[o], __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT) < round && --budget > 0)
              __builtin_amdgcn_s_sleep(1);
            lost = lost || budget <= 0;     // the partner never published this round: its slot holds an older round's records
            const unsigned long long* theirs = reinterpret_cast<const unsigned long long*>(slot0 + o * 512 + l_ * 8);
            const unsigned long long w0 = __hip_atomic_load(theirs + 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            const unsigned long long w1 = __hip_atomic_load(theirs + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            const unsigned long long w2 = __hip_atomic_load(theirs + 2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            ov = __uint_as_float((unsigned)w0); ov2 = __uint_as_float((unsigned)(w0 >> 32));
            orp = make_float4(__uint_as_float((unsigned)w1), __uint_as_float((unsigned)(w1 >> 32)),
                              __uint_as_float((unsigned)w2), __uint_as_float((unsigned)(w2 >> 32)));
          }
          const bool better = ov > bv;
          rest = vmax_f32(rest, better ? bv : ov);
          bv2 = better ? ov2 : bv2;
          brp.x = better ? orp.x : brp.x; brp.y = better ? orp.y : brp.y;
          brp.z = better ? orp.z : brp.z; brp.w = better ? orp.w : brp.w;
          bv = better ? ov : bv;
        }
        v = bv;
        v2 = vmax_f32(rest, bv2);
        rp = brp;
      }
      // Candidates: the lanes above a threshold tau (adaptive: any tau is correct, it only decides how many there are).
      // B bounds every point that is NOT a surviving candidate: the other lanes' best values, the candidates' own second
      // bests, and the candidates that do not beat it.  The survivors A, taken in descending order, are the next picks for as
      // long as each is untouched by the ones before it (and no two are equal) -- all lanes evaluate that in parallel.
      const float m0 = wave_max_fast(v);
      float tau = m0 * rho;
      unsigned long long cm = __ballot(v > tau);
      int ncand = (int)__popcll(cm);
#pragma unroll 1
      for (int t = 0; t < 4 && ncand > 16; ++t) {
        tau = 0.5f * (tau + m0);
        cm = __ballot(v > tau);
        ncand = (int)__popcll(cm);
      }
      if (ncand > 16) cm = __ballot(v == m0);
      rho = ncand > 16 ? 0.5f * (1.f + rho) : (ncand < KP ? fmaxf(rho * rho, 0.25f) : rho);
      rho = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, rho)));   // uniform: an SGPR
      const bool cand = (cm >> l_) & 1ull;
      const float B = wave_max_fast(cand ? v2 : v);
      unsigned long long am = m0 > 0.f ? __ballot(cand && v > B) : 0ull;
      if (__popcll(am) > 16) am = 0ull;   // (more than 16 lanes tied at the maximum: the exact one-pick path; cand_p holds 16)
      // pairwise: the survivors are compacted into LDS (at most 16), lane l looks at the pairs (j = l % 16, i = l / 16 + 4 t):
      // how many survivors precede j (rank), does one of them touch it or equal it (bad)
      const int n_a = (int)__popcll(am);
      const bool in_a = (am >> l_) & 1ull;
      const int pos = (int)__popcll(am & ((1ull << l_) - 1ull));
      if (in_a) {
        cand_p[pos] = make_float4(rp.x, rp.y, rp.z, v);
        cand_q[pos] = __float_as_int(rp.w);
      }
      const int j = l_ & 15, ig = l_ >> 4;
      const float4 cj = cand_p[j];
      int rank_part = 0;
      bool bad_part = false;
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const int i2 = ig + 4 * t;
        const float4 ci = cand_p[i2];
        const bool live = i2 < n_a && j < n_a && i2 != j;
        const bool higher = ci.w > cj.w;                      // survivor i2 is picked before j
        rank_part += live && higher ? 1 : 0;
        bad_part = bad_part || (live && (ci.w == cj.w || (higher && sqdist3(cj.x, cj.y, cj.z, ci.x, ci.y, ci.z) < cj.w)));
      }
      rank_buf[l_] = rank_part;
      const unsigned long long bm = __ballot(bad_part);
      const bool bad = (((bm | (bm >> 16) | (bm >> 32) | (bm >> 48)) >> j) & 1ull) != 0ull;
      const int rank = rank_buf[j] + rank_buf[j + 16] + rank_buf[j + 32] + rank_buf[j + 48];     // lanes 0..15: survivor j
      const bool mine = l_ < n_a;                             // from here on lane j < n_a speaks for survivor j
      const int bad_rank = (int)-wave_max_fast(mine && bad ? -(float)rank : -99.f);
      const int cnt = min(min(n_a, bad_rank), min(KP, M - i));
      if (mine && rank < cnt) {
        accb[rank] = make_float4(cj.x, cj.y, cj.z, __int_as_float(cand_q[l_]));
        picks[i + rank] = cand_q[l_];                    // sorted position; translated to the original index after the loop
      }
      if constexpr (MULTI) {
        // a lost partner: the replicated selection would diverge between the scene's workgroups from here on.  Flag the
        // launch (the host raises when it next looks: pn2_ext.raise_if_fps_failed) and leave the round loop.
        if (__any(lost)) {
          if (l_ == 0) { atomicOr(status, 1u); acc_n = -1; }
        } else if (l_ == 0) { acc_n = cnt; fb_mx = m0; }
      } else {
        if (l_ == 0) { acc_n = cnt; fb_mx = m0; }
      }
    }
    __syncthreads();
    const int got = __builtin_amdgcn_readfirstlane(acc_n);
    if (MULTI && got < 0) break;            // (uniform: acc_n is the workgroup's)
    if (got > 0) {
      i += got;
      continue;
    }
    // ---- exact one-pick path (equal maxima / all distances zero): the reference's tie order through the keys ------------
    const float mx = fb_mx;
    if (mx > 0.f) {
      unsigned kmin = 0xffffffffu;
      int nm = 0;
      FPS_SLOTS(FPS_SLOT_FALLBACK)
      if (kmin != 0xffffffffu) { atomicMin(&win_key, kmin); atomicAdd(&tie_cnt, nm); }
    }
    __syncthreads();
    if constexpr (MULTI) {
      // the smallest key of all workgroups: one 64-bit word each (round << 32 | key), same tag discipline as the records
      if (tid == 0) {
        unsigned long long* const kslot = keyw + (round & 1u) * 4u;
        __hip_atomic_store(&kslot[h], ((unsigned long long)round << 32) | win_key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        unsigned kall = win_key;
        for (int o = 0; o < G; ++o) {
          if (o == h) continue;
          unsigned long long wv = 0;
          int budget = 1 << 22;
          do {
            wv = __hip_atomic_load(&kslot[o], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if ((unsigned)(wv >> 32) == round) break;
            __builtin_amdgcn_s_sleep(1);
          } while (--budget > 0);
          if (budget <= 0) { atomicOr(status, 1u); kall = FPS_LOST_KEY; break; }
          kall = min(kall, (unsigned)wv);
        }
        win_key = kall;
      }
      __syncthreads();
    }
    const unsigned key = win_key;
    __syncthreads();
    if (MULTI && key == FPS_LOST_KEY) break;
    if (tid == 0) {
      // a pick of this path is a unique strict maximum only if exactly ONE point held it (the multi-pick rounds accept
      // nothing else by construction); several holders, or all distances zero, is where a run over the picks could differ.
      // Cooperating workgroups only see their own holders: every pick of this path counts there (it is rare)
      if (MULTI || tie_cnt != 1) tie_at = min(tie_at, i);
      tie_cnt = 0;
      win_key = 0xffffffffu;
      if (key != 0xffffffffu) {
        const int cur1 = fps_unkey(key, rb_log2);
        accb[0] = make_float4(base[(int64_t)cur1 * sn], base[sc + (int64_t)cur1 * sn], base[2 * sc + (int64_t)cur1 * sn],
                              __int_as_float(-1));
        picks[i] = -cur1 - 1;             // already an original index
      } else {
        picks[i] = picks[i - 1];          // all distances 0: the reference repeats its last pick (accb[0] may stay what it is:
      }                                   // its distances are all zero already, nothing can change)
      acc_n = 1;
    }
    i += 1;
    __syncthreads();
  }
  // the round loop touches no global memory of its own (a store in front of a barrier costs its acknowledgement, ~1 us per
  // round): the picks wait in LDS as codes and are translated here -- by the workgroup that owns the point
  for (int k = tid; k < M; k += T) {
    const int v = picks[k];
    if (v < 0) {
      if (h == 0) out[k] = (int64_t)(-v - 1);
    } else if ((v >> 24) == h) {
      out[k] = (int64_t)n0 + (int64_t)perm[v & 0xffffff];
    }
  }
  if (first_tie && tid == 0 && h == 0) first_tie[b] = tie_at;
}

// Fallback for scenes too large to keep resident: min-distances live in a caller-provided
// (B,N) workspace, xyz is re-read (L2) each round.  Same tie order.
template <int T>
__global__ __launch_bounds__(T) void fps_streaming_kernel(const float* __restrict__ xyz, int64_t sb, int64_t sc,
                                                          int64_t sn, int N, int M, int rb_log2,
                                                          float* __restrict__ temp, int64_t* __restrict__ index) {
  constexpr int W = T / 64;
  __shared__ unsigned long long part[2][W];
  const int tid = threadIdx.x;
  const float* base = xyz + (int64_t)blockIdx.x * sb;
  float* tmp = temp + (int64_t)blockIdx.x * N;
  int64_t* out = index + (int64_t)blockIdx.x * M;
  for (int j = tid; j < N; j += T) tmp[j] = __builtin_inff();
  if (tid == 0) out[0] = 0;
  int cur = 0;
  for (int i = 1; i < M; ++i) {
    const float cx = base[(int64_t)cur * sn];
    const float cy = base[sc + (int64_t)cur * sn];
    const float cz = base[2 * sc + (int64_t)cur * sn];
    float best = 0.f;
    int best_j = cur;
    for (int j = tid; j < N; j += T) {
      float d = sqdist3(base[(int64_t)j * sn], base[sc + (int64_t)j * sn], base[2 * sc + (int64_t)j * sn], cx, cy, cz);
      float nd = fminf(tmp[j], d);
      tmp[j] = nd;
      if (nd > best) { best = nd; best_j = j; }
    }
    unsigned long long packed =
        ((unsigned long long)__float_as_uint(best) << 32) | (unsigned long long)(~fps_key(best_j, rb_log2));
    packed = wave_max_u64(packed);
    if ((tid & 63) == 0) part[i & 1][tid >> 6] = packed;
    __syncthreads();
    unsigned long long m = part[i & 1][0];
#pragma unroll
    for (int w = 1; w < W; ++w) {
      unsigned long long o = part[i & 1][w];
      m = o > m ? o : m;
    }
    cur = __builtin_amdgcn_readfirstlane(fps_unkey(~(unsigned)(m & 0xffffffffull), rb_log2));
    if (tid == 0) out[i] = cur;
  }
}

// Scenes too large for one CU's register file (25 600 < N <= 102 400): G = 2..4 workgroups per scene, each keeping an
// interleaved share of the points resident exactly like fps_resident_kernel (workgroup h holds j = (s G + h) T + tid, so a
// thread's points still share one reference lane and its slot order is the reference's order), plus one exchange per round
// through a few words of global memory: every workgroup publishes its local (maximum, tie-break key) as ONE 64-bit word
//   [ distance bits : 32 | round tag : 15 | 0x1ffff - compact key : 17 ]
// in slot [scene][round & 1][h] and polls the others' slots until their tag is this round's; the largest word wins
// (largest distance, then smallest key).  Double buffering by round parity is enough: a workgroup can only run one
// round ahead of the slowest.  The workgroups of a scene are co-resident by construction (a launch needs G B <= #CUs
// whole CUs) and are mapped to one XCD when B % 8 == 0 so the words stay in one L2.  ~4 us per round instead of the
// streaming kernel's 27 us.  A poll budget turns a (never observed) lost partner into garbage output instead of a hang.
__device__ __forceinline__ unsigned fps_compact_key(unsigned key, int rb_log2) {   // order-preserving, < 2^17 for N < 2^17
  const unsigned hi_mask = ~(0xffffffffu >> rb_log2);
  return ((key & hi_mask) >> (32 - 17)) | (key & ~hi_mask);   // reversed lane -> bits [17-rb, 17), j / RB below
}
__device__ __forceinline__ unsigned fps_expand_key(unsigned ckey, int rb_log2) {
  const unsigned lo_mask = (1u << (17 - rb_log2)) - 1u;
  return ((ckey & ~lo_mask) << (32 - 17)) | (ckey & lo_mask);
}

template <int PPT>
__global__ __launch_bounds__(1024) void fps_multi_kernel(const float* __restrict__ xyz, int64_t sb, int64_t sc, int64_t sn,
                                                         int N, int M, int rb_log2, int G, int B, int Bpad,
                                                         unsigned long long* __restrict__ slots,
                                                         int64_t* __restrict__ index) {
  constexpr int T = 1024, W = T / 64, WP = W;
  __shared__ __attribute__((aligned(16))) float part[2][WP];
  __shared__ unsigned win_key[2];
  __shared__ unsigned long long xchg[4];
  const int tid = threadIdx.x;
  const int b = (int)(blockIdx.x % (unsigned)Bpad), h = (int)(blockIdx.x / (unsigned)Bpad);
  if (b >= B) return;
  const float* base = xyz + (int64_t)b * sb;
  int64_t* out = index + (int64_t)b * M;
  unsigned long long* my_slots = slots + (int64_t)b * 8;   // [parity][h], h < 4

  float px[PPT], py[PPT], pz[PPT], dist[PPT];
#pragma unroll
  for (int s = 0; s < PPT; ++s) {
    const int j = (s * G + h) * T + tid;
    if (j < N) {
      px[s] = base[(int64_t)j * sn];
      py[s] = base[sc + (int64_t)j * sn];
      pz[s] = base[2 * sc + (int64_t)j * sn];
      dist[s] = __builtin_inff();
    } else {
      px[s] = py[s] = pz[s] = 0.f;
      dist[s] = -1.f;
    }
  }
  if (tid < 2 * WP) (&part[0][0])[tid] = 0.f;
  if (tid < 2) win_key[tid] = 0xffffffffu;
  if (tid == 0 && h == 0) out[0] = 0;
  __syncthreads();
  int cur = 0;
  for (int i = 1; i < M; ++i) {
    const int buf = i & 1;
    const float cx = base[(int64_t)cur * sn];
    const float cy = base[sc + (int64_t)cur * sn];
    const float cz = base[2 * sc + (int64_t)cur * sn];
    float tmax = 0.f;
#pragma unroll
    for (int s = 0; s < PPT; ++s) {
      const float nd = vmin_f32(dist[s], sqdist3(px[s], py[s], pz[s], cx, cy, cz));
      dist[s] = nd;
      tmax = fmaxf(tmax, nd);
    }
    const float wmax = wave_max_f32(tmax);
    if ((tid & 63) == 0) part[buf][tid >> 6] = wmax;
    __syncthreads();
    if (tid == 0) win_key[buf ^ 1] = 0xffffffffu;   // after the barrier: see fps_resident_kernel
    float mx = 0.f;
#pragma unroll
    for (int w4 = 0; w4 < WP / 4; ++w4) {
      const float4 q = *reinterpret_cast<const float4*>(&part[buf][w4 * 4]);
      mx = fmaxf(fmaxf(mx, fmaxf(q.x, q.y)), fmaxf(q.z, q.w));
    }
    if (mx > 0.f && tmax == mx) {
      int best_s = 0;
#pragma unroll
      for (int s = PPT - 1; s >= 0; --s)
        if (dist[s] == mx) best_s = s;
      atomicMin(&win_key[buf], fps_key((best_s * G + h) * T + tid, rb_log2));
    }
    __syncthreads();
    // ---- exchange with the other workgroups of this scene -------------------------------------------------------------
    const unsigned tag = (unsigned)i & 0x7fffu;
    if (tid == 0) {
      const unsigned key = win_key[buf];
      const unsigned inv = key == 0xffffffffu ? 0u : 0x1ffffu - fps_compact_key(key, rb_log2);
      const unsigned long long word = ((unsigned long long)__float_as_uint(mx) << 32) | ((unsigned long long)tag << 17) | inv;
      xchg[h] = word;
      __hip_atomic_store(&my_slots[buf * 4 + h], word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    } else if (tid >= 64 && tid < 64 + G && tid - 64 != h) {   // one lane of ANOTHER wave per partner: inside one wave
      const int o = tid - 64;                                  // the poll branch could be scheduled ahead of the store
      unsigned long long wv = 0;
      int budget = 1 << 22;
      do {
        wv = __hip_atomic_load(&my_slots[buf * 4 + o], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if ((unsigned)((wv >> 17) & 0x7fffu) == tag) break;
        __builtin_amdgcn_s_sleep(1);
      } while (--budget > 0);
      xchg[o] = wv;
    }
    __syncthreads();
    unsigned long long best = xchg[0];
    for (int o = 1; o < G; ++o) best = xchg[o] > best ? xchg[o] : best;
    const unsigned inv = (unsigned)(best & 0x1ffffull);
    if ((best >> 32) != 0ull && inv != 0u)   // else: every distance is 0 -> repeat cur
      cur = fps_unkey(fps_expand_key(0x1ffffu - inv, rb_log2), rb_log2);
    cur = __builtin_amdgcn_readfirstlane(cur);
    if (tid == 0 && h == 0) out[i] = cur;
  }
}

static int ref_block_log2(int64_t n) {  // csrc/sampling_kernel.cu:32-40 + the >=16 switch (:148-165)
  int cnt = 0;
  int64_t x = n - 1;
  while (x > 0) { x >>= 1; ++cnt; }
  if (cnt > 9) cnt = 9;
  if (cnt < 4) cnt = 4;
  return cnt;
}

#define FPS_RESIDENT_MAX 25600
#define FPS_MULTI_MAX (4 * FPS_RESIDENT_MAX)

static int fps_num_cus() {
  static int n = 0;
  if (n == 0) {
    int dev = 0, v = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess ||
        v <= 0)
      v = 256;
    n = v;
  }
  return n;
}

// Measurement switches: inputs of fps_plan and of nothing else.
#ifndef FPS_CLUSTERS
#define FPS_CLUSTERS 1   // 1: fps_cluster_kernel (pruning per 64-point cluster); 0: fps_sorted_kernel (per wave)
#endif
#ifndef FPS_COOP
#define FPS_COOP 1       // 1: scenes beyond 25 600 points sample with fps_cluster_kernel<.., true> (several picks per exchange)
#endif
#ifndef FPS_COOP_MIN_N
#define FPS_COOP_MIN_N FPS_RESIDENT_MAX   // scenes with MORE points sample on cooperating workgroups ...
#endif
#ifndef FPS_COOP_SLICE
#define FPS_COOP_SLICE FPS_RESIDENT_MAX   // ... ceil(N / this) of them (measurement builds lower both: scripts/fps_coop_probe.py)
#endif
#ifndef FPS_CLUSTER_MIN_PICKS_SMALL
#define FPS_CLUSTER_MIN_PICKS_SMALL 512   // 4096 < N <= 8192: runs at least this long take the cluster kernel too
#endif
#ifndef FPS_CLUSTER_PICKS
#define FPS_CLUSTER_PICKS 8
#endif

// The points-per-thread ladder: a scene (or a cooperating workgroup's slice of one) of up to `n` points is held by `threads`
// threads with `ppt` points each.  The in-thread scan keeps the first strict maximum in slot order; that equals the reference's
// order only if all points of a thread share one reference lane (j mod RB), i.e. T % RB == 0 or one point per thread.  Hence
// T = RB (PPT 1) up to 512 points and T in {512, 1024} above.
struct FpsTile { int n, threads, ppt; };
static constexpr FpsTile fps_tiles[] = {{64, 64, 1},      {128, 128, 1},    {256, 256, 1},    {512, 512, 1},   {1024, 512, 2},
                                        {2048, 512, 4},   {4096, 512, 8},   {6144, 1024, 6},  {8192, 1024, 8}, {12288, 1024, 12},
                                        {16384, 1024, 16}, {20480, 1024, 20}, {FPS_RESIDENT_MAX, 1024, 25}};
enum { FPS_TILES = sizeof(fps_tiles) / sizeof(fps_tiles[0]) };
static_assert(FPS_COOP_SLICE <= FPS_RESIDENT_MAX, "a slice is held by one workgroup");

// The one place a run-time row of fps_tiles becomes template arguments: f(std::integral_constant<int, tile>), false if f
// launched nothing.
template <class F, int... I>
static bool fps_with_tile(int tile, F f, std::integer_sequence<int, I...>) {
  return ((tile == I && f(std::integral_constant<int, I>{})) || ...);
}

// kernel families, regnet_fps_plan's [0]: from FPS_FAM_COOP up a launch wants the exchange area's bytes
enum { FPS_FAM_NONE = 0, FPS_FAM_RESIDENT, FPS_FAM_CLUSTER, FPS_FAM_SORTED, FPS_FAM_COOP, FPS_FAM_MULTI, FPS_FAM_STREAMING };
// by family: the first row of fps_tiles its kernel is instantiated for (the plan takes no smaller one, the launch compiles no other)
static constexpr int fps_first_tile[] = {0, 0, 7, 9, 9, FPS_TILES - 1, FPS_TILES - 1};

// What (B, N, M) takes, regnet_fps_plan's words (include/regnet_hip.h) with the row of fps_tiles in place of [1] and [2].
struct FpsPlan {
  int family, tile, G, Bpad;
  int64_t grid, ws_bytes, xchg_off, status_off;
};

// The only place that knows the thresholds; no device pointer, no stream.  Returns what fps_launch returns for these sizes
// before it looks at a pointer.
static int fps_plan(int64_t B, int64_t N, int64_t M, FpsPlan& p) {
  p = FpsPlan{};
  p.xchg_off = p.status_off = -1;
  if (M <= 0 || N < M || B < 0) return REGNET_ERR_SHAPE;
  if (N >= (int64_t)1 << 30) return REGNET_ERR_UNSUPPORTED;
  if (B == 0) return REGNET_OK;
  const int64_t Gc = (N + FPS_COOP_SLICE - 1) / FPS_COOP_SLICE, Gm = (N + FPS_RESIDENT_MAX - 1) / FPS_RESIDENT_MAX;
  // the counting-sort prologue of the sorting kernels costs ~0.7 ms: only worth it for long runs (4096 < N <= 8192 is level 2
  // of the network: 1024 picks of 5120 points)
  const bool long_run = N > 8192 ? M >= 1024 : N > 4096 && FPS_CLUSTERS && M >= FPS_CLUSTER_MIN_PICKS_SMALL;
  const bool fits_lds = M <= FPS_CLUSTER_MAX_PICKS;   // fps_cluster_kernel keeps the picks of one launch in LDS
  p.G = 1;
  if (FPS_CLUSTERS && FPS_COOP && N > FPS_COOP_MIN_N && N <= FPS_MULTI_MAX && M >= 1024 && fits_lds && Gc <= 4 &&
      Gc * B <= fps_num_cus()) {
    // several exact picks per round on 2..4 cooperating workgroups per scene (fps_cluster_kernel<.., true>)
    p.family = FPS_FAM_COOP; p.G = (int)Gc;
  } else if (N <= FPS_RESIDENT_MAX) {
    p.family = !long_run ? FPS_FAM_RESIDENT : FPS_CLUSTERS && fits_lds ? FPS_FAM_CLUSTER : FPS_FAM_SORTED;
  } else if (N <= FPS_MULTI_MAX && M < 32768 /* 15-bit round tag */ && Gm * B <= fps_num_cus()) {
    p.family = FPS_FAM_MULTI; p.G = (int)Gm;   // 2..4 workgroups (whole CUs) per scene
  } else {
    p.family = FPS_FAM_STREAMING;              // running distances in the workspace, any N
  }
  // the points one workgroup holds in registers (the multi-workgroup and streaming kernels: always the last row)
  for (p.tile = fps_first_tile[p.family]; p.tile < FPS_TILES - 1 && fps_tiles[p.tile].n < (N + p.G - 1) / p.G; ++p.tile) {}
  p.Bpad = p.G > 1 ? (int)((B + 7) / 8 * 8) : (int)B;
  p.grid = (int64_t)p.Bpad * p.G;
  const int64_t words = B * N * (int64_t)sizeof(float);
  if (p.family == FPS_FAM_CLUSTER) p.ws_bytes = words;
  if (p.family >= FPS_FAM_COOP) {   // beyond one CU: the exchange area, 16-byte aligned behind the B x N words, and the status word
    const int64_t behind = (words + 15) / 16 * 16;
    p.ws_bytes = behind + B * (int64_t)FPS_XCHG_BYTES + FPS_STATUS_BYTES;
    if (p.family == FPS_FAM_COOP) { p.xchg_off = behind; p.status_off = behind + B * (int64_t)FPS_XCHG_BYTES; }
    if (p.family == FPS_FAM_MULTI) p.xchg_off = 0;   // 64 bytes per scene at the front: it keeps no B x N words
  }
  return REGNET_OK;
}

extern "C" int regnet_fps_plan(int64_t B, int64_t N, int64_t M, int64_t* plan) {
  if (!plan) return REGNET_ERR_NULL;
  FpsPlan p;
  const int rc = fps_plan(B, N, M, p);
  const FpsTile t = p.family == FPS_FAM_NONE ? FpsTile{} : fps_tiles[p.tile];
  const int64_t out[9] = {p.family, t.threads, p.family == FPS_FAM_STREAMING ? 0 : t.ppt, p.G, p.Bpad, p.grid, p.ws_bytes,
                          p.xchg_off, p.status_off};
  for (int i = 0; i < 9; ++i) plan[i] = rc == REGNET_OK ? out[i] : 0;
  return rc;
}

static FpsPlan fps_plan_of(int64_t B, int64_t N, int64_t M) { FpsPlan p; fps_plan(B, N, M, p); return p; }
extern "C" int64_t regnet_fps_workspace_bytes(int64_t B, int64_t N, int64_t M) { return fps_plan_of(B, N, M).ws_bytes; }
extern "C" int64_t regnet_fps_status_offset_bytes(int64_t B, int64_t N, int64_t M) { return fps_plan_of(B, N, M).status_off; }

static int fps_launch(const float* xyz, int64_t sb, int64_t sc, int64_t sn, int64_t B, int64_t N, int64_t M, int64_t* index,
                      float* workspace, const int* prefix_ok, int* first_tie, void* stream) {
  FpsPlan p;
  const int rc = fps_plan(B, N, M, p);
  if (rc != REGNET_OK || B == 0) return rc;
  if (!xyz || !index || (p.ws_bytes > 0 && !workspace)) return REGNET_ERR_NULL;
  hipStream_t st = as_stream(stream);
  hipError_t e = hipSuccess;
  if (p.family == FPS_FAM_COOP)    // tags 0 = nothing published, status 0 = no poll gave up
    e = hipMemsetAsync(workspace + p.xchg_off / 4, 0, (size_t)B * FPS_XCHG_BYTES + FPS_STATUS_BYTES, st);
  if (p.family == FPS_FAM_MULTI) e = hipMemsetAsync(workspace, 0, (size_t)B * 64, st);   // round tag 0 = "nothing published"
  if (e != hipSuccess) return (int)e;
  if (first_tie && p.family >= FPS_FAM_MULTI &&   // (no tie tracking, no shortcut: "unknown")
      (e = hipMemsetAsync(first_tie, 0, (size_t)B * sizeof(int), st)) != hipSuccess)
    return (int)e;
  const int rbl = ref_block_log2(N), n = (int)N, m = (int)M, b = (int)B;
  const dim3 grid((unsigned)p.grid), block((unsigned)fps_tiles[p.tile].threads);
  unsigned* const perm = reinterpret_cast<unsigned*>(workspace);                        // the sort's permutation: B x N words
  float* const xchg = p.family == FPS_FAM_COOP ? workspace + p.xchg_off / 4 : nullptr;
  // every launch starts with the same arguments; a family's kernel exists from fps_first_tile up
#define FPS_LAUNCH(FAMILY, KERNEL, ...)                                                                              \
  case FAMILY:                                                                                                       \
    if constexpr (tile < fps_first_tile[FAMILY]) return false;                                                       \
    else { hipLaunchKernelGGL(KERNEL, grid, block, 0, st, xyz, sb, sc, sn, n, m, rbl, __VA_ARGS__); return true; }
  const bool launched = fps_with_tile(p.tile, [&](auto I) {
    constexpr int tile = decltype(I)::value;
    constexpr FpsTile t = fps_tiles[tile];
    switch (p.family) {
      FPS_LAUNCH(FPS_FAM_RESIDENT, (fps_resident_kernel<t.threads, t.ppt>), index, prefix_ok, first_tie)
      FPS_LAUNCH(FPS_FAM_SORTED, (fps_sorted_kernel<t.ppt, FPS_PICKS>), index, prefix_ok, first_tie)
#if FPS_CLUSTERS
      FPS_LAUNCH(FPS_FAM_CLUSTER, (fps_cluster_kernel<t.ppt, FPS_CLUSTER_PICKS, false>), perm, index, p.G, b, p.Bpad, xchg,
                 prefix_ok, first_tie)
      FPS_LAUNCH(FPS_FAM_COOP, (fps_cluster_kernel<t.ppt, FPS_CLUSTER_PICKS, true>), perm, index, p.G, b, p.Bpad, xchg,
                 prefix_ok, first_tie)
#endif
      FPS_LAUNCH(FPS_FAM_MULTI, (fps_multi_kernel<t.ppt>), p.G, b, p.Bpad, (unsigned long long*)workspace, index)
      FPS_LAUNCH(FPS_FAM_STREAMING, (fps_streaming_kernel<t.threads>), workspace, index)
    }
    return false;
  }, std::make_integer_sequence<int, FPS_TILES>{});
  if (!launched) return REGNET_ERR_UNSUPPORTED;   // a (family, tile) no kernel is compiled for: never OK with index unwritten
  REGNET_LAUNCH_CHECK();
  return REGNET_OK;
}

extern "C" int regnet_fps_f32(const float* xyz, int64_t sb, int64_t sc, int64_t sn, int64_t B, int64_t N, int64_t M,
                              int64_t* index, float* workspace, void* stream) {
  return fps_launch(xyz, sb, sc, sn, B, N, M, index, workspace, nullptr, nullptr, stream);
}

extern "C" int regnet_fps_chain_f32(const float* xyz, int64_t sb, int64_t sc, int64_t sn, int64_t B, int64_t N, int64_t M,
                                    int64_t* index, float* workspace, const int32_t* prefix_ok, int32_t* first_tie,
                                    void* stream) {
  return fps_launch(xyz, sb, sc, sn, B, N, M, index, workspace, prefix_ok, first_tie, stream);
}

// =====================================================================================
// Ball query
// =====================================================================================
// A wave owns BQ_CPW centroids at once (their xyz are wave-uniform); the workgroup streams
// the scene through LDS in tiles (SoA, coalesced fill), each lane tests one staged point
// against the wave's centroids, and hits are appended in index order with a ballot +
// prefix-popcount.  A wave stops at the first tile boundary after all its centroids have
// K hits (the reference's per-thread early exit, ball_query_kernel.cu:55).
#define BQ_WAVES 4
#define BQ_CPW 4
#define BQ_TILE 1024

__global__ __launch_bounds__(BQ_WAVES * 64) void ball_query_kernel(
    const float* __restrict__ xyz, int64_t sb, int64_t sc, int64_t sn, const float* __restrict__ ctr, int64_t cb,
    int64_t cc, int64_t cn, int N1, int N2, float r2, int K, int64_t* __restrict__ index,
    int64_t* __restrict__ count) {
  __shared__ float tx[BQ_TILE], ty[BQ_TILE], tz[BQ_TILE];
  __shared__ int wave_done[BQ_WAVES];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int b = blockIdx.y;
  const float* base = xyz + (int64_t)b * sb;
  const float* cbase = ctr + (int64_t)b * cb;
  const int c0 = (blockIdx.x * BQ_WAVES + wave) * BQ_CPW;

  float cx[BQ_CPW], cy[BQ_CPW], cz[BQ_CPW];
  int cnt[BQ_CPW], first[BQ_CPW];
#pragma unroll
  for (int q = 0; q < BQ_CPW; ++q) {
    int c = c0 + q;
    bool ok = c < N2;
    int cs = ok ? c : 0;
    cx[q] = cbase[(int64_t)cs * cn];
    cy[q] = cbase[cc + (int64_t)cs * cn];
    cz[q] = cbase[2 * cc + (int64_t)cs * cn];
    cnt[q] = ok ? 0 : K;  // out-of-range centroids are "already full"
    first[q] = 0;
  }
  if (lane == 0) wave_done[wave] = 0;
  const unsigned long long lt_mask = (1ull << lane) - 1ull;

  for (int t0 = 0; t0 < N1; t0 += BQ_TILE) {
    __syncthreads();  // previous tile fully consumed (also publishes wave_done)
    bool all_done = true;
#pragma unroll
    for (int w = 0; w < BQ_WAVES; ++w) all_done = all_done && (wave_done[w] != 0);
    if (all_done) break;
    for (int p = tid; p < BQ_TILE; p += BQ_WAVES * 64) {
      int j = t0 + p;
      if (j < N1) {
        tx[p] = base[(int64_t)j * sn];
        ty[p] = base[sc + (int64_t)j * sn];
        tz[p] = base[2 * sc + (int64_t)j * sn];
      }
    }
    __syncthreads();
    const int tile_n = min(BQ_TILE, N1 - t0);
    bool mine_done = true;
#pragma unroll
    for (int q = 0; q < BQ_CPW; ++q) mine_done = mine_done && (cnt[q] >= K);
    if (!mine_done) {
      for (int p0 = 0; p0 < tile_n; p0 += 64) {
        const int p = p0 + lane;
        const bool valid = p < tile_n;
        const float x = valid ? tx[p] : 0.f, y = valid ? ty[p] : 0.f, z = valid ? tz[p] : 0.f;
        const int j = t0 + p;
#pragma unroll
        for (int q = 0; q < BQ_CPW; ++q) {
          if (cnt[q] < K) {  // wave-uniform
            float d = sqdist3(x, y, z, cx[q], cy[q], cz[q]);
            bool hit = valid && (d < r2);
            unsigned long long mask = __ballot(hit);
            if (mask) {
              if (cnt[q] == 0) first[q] = t0 + p0 + (int)__builtin_ctzll(mask);
              int pos = cnt[q] + (int)__popcll(mask & lt_mask);
              if (hit && pos < K) index[((int64_t)b * N2 + (c0 + q)) * K + pos] = j;
              cnt[q] = min(K, cnt[q] + (int)__popcll(mask));
            }
          }
        }
      }
      mine_done = true;
#pragma unroll
      for (int q = 0; q < BQ_CPW; ++q) mine_done = mine_done && (cnt[q] >= K);
      if (mine_done && lane == 0) wave_done[wave] = 1;
    }
  }
  // tail: slots [cnt, K) repeat the first hit (or 0 for an empty ball); write counts.
#pragma unroll
  for (int q = 0; q < BQ_CPW; ++q) {
    int c = c0 + q;
    if (c < N2) {
      for (int k = cnt[q] + lane; k < K; k += 64) index[((int64_t)b * N2 + c) * K + k] = first[q];
      if (lane == 0) count[(int64_t)b * N2 + c] = cnt[q];
    }
  }
}

extern "C" int regnet_ball_query_f32(const float* xyz, int64_t sb, int64_t sc, int64_t sn, const float* centroids,
                                     int64_t cb, int64_t cc, int64_t cn, int64_t B, int64_t N1, int64_t N2,
                                     float radius, int64_t K, int64_t* index, int64_t* count, void* stream) {
  if (K <= 0 || B < 0 || N1 < 0 || N2 < 0) return REGNET_ERR_SHAPE;
  if (N1 >= (int64_t)1 << 31 || N2 >= (int64_t)1 << 31 || K >= (int64_t)1 << 20 || B > 65535)
    return REGNET_ERR_UNSUPPORTED;
  if (B == 0 || N2 == 0) return REGNET_OK;
  if (!centroids || !index || !count || (N1 > 0 && !xyz)) return REGNET_ERR_NULL;
  const float r2 = radius * radius;  // fp32, as ball_query_kernel.cu:47
  const int per_block = BQ_WAVES * BQ_CPW;
  dim3 grid((unsigned)((N2 + per_block - 1) / per_block), (unsigned)B);
  hipLaunchKernelGGL(ball_query_kernel, grid, dim3(BQ_WAVES * 64), 0, as_stream(stream), xyz, sb, sc, sn, centroids,
                     cb, cc, cn, (int)N1, (int)N2, r2, (int)K, index, count);
  REGNET_LAUNCH_CHECK();
  return REGNET_OK;
}

// =====================================================================================
// 3-NN search
// =====================================================================================
// One thread per query; the key set streams through LDS as float4 (x,y,z,-) and every lane
// reads the same LDS address (broadcast, conflict-free).  Sorted 3-slot insertion with
// strict <, so the earlier key index wins ties (interpolate_kernel.cu:59-69).  The
// reference's {1e40,0,0} initialiser is equivalent to {inf,inf,inf} once N2 >= 3 keys have
// been inserted (enforced at interpolate_kernel.cu:102 and here).
#define NN_THREADS 256
#define NN_TILE 2048

__global__ __launch_bounds__(NN_THREADS) void three_nn_kernel(const float* __restrict__ query, int64_t qb, int64_t qc,
                                                              int64_t qn, const float* __restrict__ key, int64_t kb,
                                                              int64_t kc, int64_t kn, int N1, int N2,
                                                              int64_t* __restrict__ index,
                                                              float* __restrict__ dist2) {
  __shared__ float4 tk[NN_TILE];
  const int tid = threadIdx.x;
  const int b = blockIdx.y;
  const int i = blockIdx.x * NN_THREADS + tid;
  const bool active = i < N1;
  const float* qbase = query + (int64_t)b * qb;
  const float* kbase = key + (int64_t)b * kb;
  const int is = active ? i : 0;
  const float qx = qbase[(int64_t)is * qn], qy = qbase[qc + (int64_t)is * qn], qz = qbase[2 * qc + (int64_t)is * qn];
  float d0 = __builtin_inff(), d1 = d0, d2 = d0;
  int i0 = -1, i1 = -1, i2 = -1;
  for (int t0 = 0; t0 < N2; t0 += NN_TILE) {
    __syncthreads();
    for (int p = tid; p < NN_TILE; p += NN_THREADS) {
      int j = t0 + p;
      if (j < N2)
        tk[p] = make_float4(kbase[(int64_t)j * kn], kbase[kc + (int64_t)j * kn], kbase[2 * kc + (int64_t)j * kn], 0.f);
    }
    __syncthreads();
    const int tile_n = min(NN_TILE, N2 - t0);
    for (int p = 0; p < tile_n; ++p) {
      const float4 k4 = tk[p];
      const float d = sqdist3(qx, qy, qz, k4.x, k4.y, k4.z);  // query minus key, as the reference
      if (d < d2) {
        const int j = t0 + p;
        const bool a = d < d0, bb = d < d1;
        d2 = bb ? d1 : d;
        i2 = bb ? i1 : j;
        d1 = a ? d0 : (bb ? d : d1);
        i1 = a ? i0 : (bb ? j : i1);
        d0 = a ? d : d0;
        i0 = a ? j : i0;
      }
    }
  }
  if (active) {
    int64_t o = ((int64_t)b * N1 + i) * 3;
    index[o + 0] = i0; index[o + 1] = i1; index[o + 2] = i2;
    dist2[o + 0] = d0; dist2[o + 1] = d1; dist2[o + 2] = d2;
  }
}

extern "C" int regnet_three_nn_f32(const float* query, int64_t qb, int64_t qc, int64_t qn, const float* key,
                                   int64_t kb, int64_t kc, int64_t kn, int64_t B, int64_t N1, int64_t N2,
                                   int64_t* index, float* dist2, void* stream) {
  if (N2 < 3 || B < 0 || N1 < 0) return REGNET_ERR_SHAPE;
  if (N1 >= (int64_t)1 << 31 || N2 >= (int64_t)1 << 31 || B > 65535) return REGNET_ERR_UNSUPPORTED;
  if (B == 0 || N1 == 0) return REGNET_OK;
  if (!query || !key || !index || !dist2) return REGNET_ERR_NULL;
  dim3 grid((unsigned)((N1 + NN_THREADS - 1) / NN_THREADS), (unsigned)B);
  hipLaunchKernelGGL(three_nn_kernel, grid, dim3(NN_THREADS), 0, as_stream(stream), query, qb, qc, qn, key, kb, kc,
                     kn, (int)N1, (int)N2, index, dist2);
  REGNET_LAUNCH_CHECK();
  return REGNET_OK;
}
