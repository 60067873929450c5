// scatter.hip -- the deterministic scatter-adds (gfx950): the backwards of group_points / gather_knn / interpolate in
// float64 (always) and in float32 under torch.use_deterministic_algorithms (the default float32 ones, gather.hip, add
// with float atomics in whatever order the hardware runs them).
//
// Contract, both dtypes: each destination element is the sum of its contributions in ascending flattened source position
// (group / gather_knn: m*K + k; interpolate: n*3 + k, adding the product g*w rounded to T), sequentially from +0.0,
// sources with an index outside [0, R) skipped -- the bits of numpy's np.add.at.  Per scene:
//   plan    -- count: contributions per destination (integer atomics: the counts do not depend on their order);
//              scan: exclusive prefix sum of the counts -> segment offsets, and a cursor per destination;
//              place: ONE wave walks the scene's sources in ascending order, 64 at a time; lanes that share a destination
//              are matched with ballots over the destination's bits, ranked with mbcnt, and the group's first lane
//              advances the destination's cursor: every segment lists its source positions in ascending order.
//              The plan depends on the indices alone: one plan serves every backward of one table.
//   segsum  -- one kernel family templated on the scalar type: the gradient rows staged in LDS when the state fits,
//              else a thread per destination reading global memory.
//
// Reference backwards (relative to multi_model/utils/pn2_utils/): group csrc/grouping_kernel.cu:103-149, interpolate
// csrc/interpolate_kernel.cu:292-337, gather_knn functions/csrc/gather_knn_kernel.cu:100-153.
//
// Built with -ffp-contract=off (csrc/build.py): no product is fused into its addition.
#include "common.h"

// =====================================================================================
// Sort plan
// =====================================================================================
// Per scene: R destinations, L sources (flattened source position p = row * inner + k, index[b, p] its destination).
// Layout (regnet_scatter_plan_bytes): cursor int32[B*R] (scratch of the placement) | offset int32[B*(R+1)] (segment of
// destination n: [offset[n], offset[n+1])) | perm int32[B*L] (the source positions of every segment, ascending).
static inline int64_t round16(int64_t x) { return (x + 15) & ~(int64_t)15; }

struct ScatterPlan {
  int* cursor;
  int* off;
  int* perm;
};

static inline ScatterPlan scatter_plan_parts(void* workspace, int64_t B, int64_t R) {
  char* ws = (char*)workspace;
  ScatterPlan p;
  p.cursor = (int*)ws;
  p.off = (int*)(ws + round16(B * R * 4));
  p.perm = (int*)(ws + round16(B * R * 4) + round16(B * (R + 1) * 4));
  return p;
}

// limits of the plan kernels (scene count, destination and source counts)
static inline bool scatter_plan_dims_ok(int64_t B, int64_t R, int64_t L) {
  return B <= 65535 && R < ((int64_t)1 << 30) && L < ((int64_t)1 << 31) && (L + 255) / 256 < ((int64_t)1 << 31);
}

#define PLAN_T 256
#define PLAN_SCAN_T 1024

__global__ __launch_bounds__(PLAN_T) void scatter_count_kernel(const int64_t* __restrict__ index, int R, int64_t L,
                                                               int* __restrict__ cnt) {
  const int b = blockIdx.y;
  const int64_t p = (int64_t)blockIdx.x * PLAN_T + threadIdx.x;
  if (p >= L) return;
  const int64_t j = index[(int64_t)b * L + p];
  if (j >= 0 && j < R) atomicAdd(&cnt[(int64_t)b * R + j], 1);
}

// one workgroup per scene: offset[n] = sum of cnt[< n], offset[R] = total; cnt becomes the placement cursor
__global__ __launch_bounds__(PLAN_SCAN_T) void scatter_scan_kernel(int* __restrict__ cnt, int R, int* __restrict__ off) {
  __shared__ int wsum[PLAN_SCAN_T / 64];
  __shared__ int carry_s;
  const int b = blockIdx.x, t = threadIdx.x, lane = t & 63, w = t >> 6;
  int* c = cnt + (int64_t)b * R;
  int* o = off + (int64_t)b * (R + 1);
  if (t == 0) carry_s = 0;
  __syncthreads();
  for (int base = 0; base < R; base += PLAN_SCAN_T) {
    const int n = base + t;
    const int v = n < R ? c[n] : 0;
    int incl = v;   // inclusive scan inside the wave
    for (int d = 1; d < 64; d <<= 1) {
      const int u = __shfl_up(incl, d, 64);
      if (lane >= d) incl += u;
    }
    if (lane == 63) wsum[w] = incl;
    __syncthreads();
    int before = carry_s;
    for (int k = 0; k < w; ++k) before += wsum[k];
    const int excl = before + incl - v;
    if (n < R) { o[n] = excl; c[n] = excl; }
    __syncthreads();
    if (t == PLAN_SCAN_T - 1) carry_s = excl + v;
    __syncthreads();
  }
  if (t == 0) o[R] = carry_s;
}

// one wave per scene, sources in ascending order: stable placement into the destinations' segments
__global__ __launch_bounds__(64) void scatter_place_kernel(const int64_t* __restrict__ index, int R, int64_t L, int nbits,
                                                           int* __restrict__ cursor, int* __restrict__ perm) {
  const int b = blockIdx.x, lane = lane_id();
  const int64_t* idx = index + (int64_t)b * L;
  int* cur = cursor + (int64_t)b * R;
  int* pm = perm + (int64_t)b * L;
  for (int64_t p0 = 0; p0 < L; p0 += 64) {
    const int64_t p = p0 + lane;
    const int64_t j = p < L ? idx[p] : -1;
    const bool valid = j >= 0 && j < R;
    const int key = valid ? (int)j : 0;
    uint64_t match = (uint64_t)__ballot(valid);
    for (int bit = 0; bit < nbits; ++bit) {
      const bool on = (key >> bit) & 1;
      const uint64_t ones = (uint64_t)__ballot(valid && on);
      match &= on ? ones : ~ones;
    }
    // (invalid lanes carry garbage in `match`; they neither lead nor place)
    const int rank = mbcnt64(match);
    const bool leader = valid && rank == 0;
    int base = 0;
    if (leader) base = atomicAdd(&cur[key], __popcll(match));
    const int leader_lane = valid ? __ffsll((unsigned long long)match) - 1 : lane;
    base = __shfl(base, leader_lane, 64);
    if (valid) pm[base + rank] = (int)p;
  }
}

// count -> scan -> place of `index` (B, L) into the plan in `workspace`; the caller checked the limits
static int build_scatter_plan(const int64_t* index, int64_t B, int64_t R, int64_t L, void* workspace, hipStream_t st) {
  ScatterPlan pl = scatter_plan_parts(workspace, B, R);
  hipError_t e = hipMemsetAsync(pl.cursor, 0, sizeof(int) * (size_t)(B * R), st);
  if (e != hipSuccess) return (int)e;
  if (L > 0) {
    hipLaunchKernelGGL(scatter_count_kernel, dim3((unsigned)((L + PLAN_T - 1) / PLAN_T), (unsigned)B), dim3(PLAN_T), 0, st,
                       index, (int)R, L, pl.cursor);
    REGNET_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(scatter_scan_kernel, dim3((unsigned)B), dim3(PLAN_SCAN_T), 0, st, pl.cursor, (int)R, pl.off);
  REGNET_LAUNCH_CHECK();
  if (L > 0) {
    int nbits = 0;
    while (((int64_t)1 << nbits) < R) ++nbits;
    hipLaunchKernelGGL(scatter_place_kernel, dim3((unsigned)B), dim3(64), 0, st, index, (int)R, L, nbits, pl.cursor,
                       pl.perm);
    REGNET_LAUNCH_CHECK();
  }
  return REGNET_OK;
}

extern "C" int64_t regnet_scatter_plan_bytes(int64_t B, int64_t num_dest, int64_t num_src) {
  if (B <= 0 || num_dest <= 0) return 0;
  if (num_src < 0) num_src = 0;
  return round16(B * num_dest * 4) + round16(B * (num_dest + 1) * 4) + round16(B * num_src * 4);
}

extern "C" int regnet_scatter_plan(const int64_t* index, int64_t B, int64_t num_dest, int64_t num_src, void* plan,
                                   void* stream) {
  if (B < 0 || num_dest < 0 || num_src < 0) return REGNET_ERR_SHAPE;
  if (B == 0 || num_dest == 0) return REGNET_OK;
  if (!scatter_plan_dims_ok(B, num_dest, num_src)) return REGNET_ERR_UNSUPPORTED;
  if (!plan || (num_src > 0 && !index)) return REGNET_ERR_NULL;
  return build_scatter_plan(index, B, num_dest, num_src, plan, as_stream(stream));
}

// =====================================================================================
// Segment sums, T = float or double
// =====================================================================================
// ---- LDS-staged --------------------------------------------------------------------------------------------------------
// A workgroup owns `cpb` channels of one scene.  It stages the gradient rows of its channels in LDS, a chunk of source
// slots at a time (one coalesced read of the gradient from HBM), and each thread walks the segments of its destinations
// through the chunk: a segment lists ascending source positions, so the part of it inside a chunk is a contiguous run
// that follows the part inside the previous chunk.  With several chunks the per-destination running sums and segment
// cursors live in LDS between chunks; with one chunk they stay in registers.
// Source slot: group / gather_knn (unweighted) the position p itself, at (p / inner) * s_hi + (p % inner) * s_lo;
// interpolate (weighted, inner = 3) the grad_out column p / 3, at (p / 3) * s_hi.
#define SEG_T 1024
#define SEG_LDS_BYTES 147456   // 144 KB: 36 864 float or 18 432 double slots
#define SEG_CH 8               // channels per workgroup at most
#define SEG_MIN_CHUNK 4096     // below this many staged slots per chunk: the global-memory kernel

template <typename T, bool WEIGHTED>
__global__ __launch_bounds__(SEG_T) void segsum_lds_kernel(const T* __restrict__ go, int64_t sb, int64_t sc, int64_t s_hi,
                                                           int64_t s_lo, int inner, int dense, const T* __restrict__ weight,
                                                           int C, int R, int64_t L, int NS, int chunk, int cpb,
                                                           const int* __restrict__ off, const int* __restrict__ perm,
                                                           T* __restrict__ gi) {
  extern __shared__ __align__(16) unsigned char seg_lds[];
  T* rows = (T*)seg_lds;                     // [cpb][chunk]
  T* acc = rows + cpb * chunk;               // [cpb][R]   (several chunks only)
  int* cur = (int*)(acc + cpb * R);          // [R]
  const int b = blockIdx.y, t = threadIdx.x;
  const int c0 = blockIdx.x * cpb, nc = min(cpb, C - c0);
  const int* o = off + (int64_t)b * (R + 1);
  const int* pm = perm + (int64_t)b * L;
  const T* wt = WEIGHTED ? weight + (int64_t)b * L : nullptr;
  const T* src = go + (int64_t)b * sb + (int64_t)c0 * sc;
  const bool multi = NS > chunk;
  if (multi) {
    for (int n = t; n < R; n += SEG_T) {
      cur[n] = o[n];
      for (int c = 0; c < nc; ++c) acc[c * R + n] = T(0);
    }
  }
  for (int s0 = 0; s0 < NS; s0 += chunk) {
    const int ns = min(chunk, NS - s0);
    __syncthreads();
    for (int i = t; i < nc * ns; i += SEG_T) {
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
    for (int n = t; n < R; n += SEG_T) {
      int i = multi ? cur[n] : o[n];
      const int end = o[n + 1];
      T a[SEG_CH];
#pragma unroll
      for (int c = 0; c < SEG_CH; ++c) a[c] = (multi && c < nc) ? acc[c * R + n] : T(0);
      for (; i < end; ++i) {
        const int p = pm[i];
        const int slot = WEIGHTED ? p / 3 : p;
        if (slot >= send) break;
        const T* r = rows + (slot - s0);
        if (WEIGHTED) {
          const T w = wt[p];
#pragma unroll
          for (int c = 0; c < SEG_CH; ++c)
            if (c < nc) {
              const T v = r[c * chunk] * w;
              a[c] = a[c] + v;
            }
        } else {
#pragma unroll
          for (int c = 0; c < SEG_CH; ++c)
            if (c < nc) a[c] = a[c] + r[c * chunk];
        }
      }
      if (multi) {
        cur[n] = i;
#pragma unroll
        for (int c = 0; c < SEG_CH; ++c)
          if (c < nc) acc[c * R + n] = a[c];
      } else {
        T* dst = gi + ((int64_t)b * C + c0) * R + n;
#pragma unroll
        for (int c = 0; c < SEG_CH; ++c)
          if (c < nc) dst[(int64_t)c * R] = a[c];
      }
    }
  }
  if (multi) {
    __syncthreads();
    T* dst = gi + ((int64_t)b * C + c0) * R;
    for (int i = t; i < nc * R; i += SEG_T) dst[i] = acc[i];
  }
}

// ---- from global memory (destination counts whose state does not fit in LDS) ------------------------------------------
// A thread per destination walks its segment in order, seg_g_ch<T> channels at a time; the grid runs the destinations of
// one channel block together so that their scattered reads share the cached gradient rows.  double takes 8 channels: with
// at most 65 535 channel blocks on grid.y it then covers every C up to 524 280.
#define SEG_G_T 256
template <typename T>
constexpr int seg_g_ch = sizeof(T) == 4 ? 4 : 8;

template <typename T>
static inline bool seg_g_channels_ok(int64_t C) {
  return (C + seg_g_ch<T> - 1) / seg_g_ch<T> <= 65535;
}

template <typename T, bool WEIGHTED>
__global__ __launch_bounds__(SEG_G_T) void segsum_global_kernel(const T* __restrict__ go, int64_t sb, int64_t sc,
                                                                int64_t s_hi, int64_t s_lo, int inner,
                                                                const T* __restrict__ weight, int C, int R, int64_t L,
                                                                const int* __restrict__ off, const int* __restrict__ perm,
                                                                T* __restrict__ gi) {
  constexpr int CH = seg_g_ch<T>;
  const int b = blockIdx.z;
  const int n = blockIdx.x * SEG_G_T + threadIdx.x;
  if (n >= R) return;
  const int c0 = blockIdx.y * CH, nc = min(CH, C - c0);
  const int* o = off + (int64_t)b * (R + 1);
  const int* pm = perm + (int64_t)b * L;
  const T* src = go + (int64_t)b * sb + (int64_t)c0 * sc;
  T a[CH];
#pragma unroll
  for (int c = 0; c < CH; ++c) a[c] = T(0);
  const int end = o[n + 1];
  for (int i = o[n]; i < end; ++i) {
    const int p = pm[i];
    const int hi = p / inner, lo = p - hi * inner;
    const T* e = src + (int64_t)hi * s_hi + (WEIGHTED ? 0 : (int64_t)lo * s_lo);
    const T w = WEIGHTED ? weight[(int64_t)b * L + p] : T(1);
#pragma unroll
    for (int c = 0; c < CH; ++c)
      if (c < nc) {
        const T g = e[(int64_t)c * sc];
        if (WEIGHTED) {
          const T v = g * w;
          a[c] = a[c] + v;
        } else {
          a[c] = a[c] + g;
        }
      }
  }
  T* dst = gi + ((int64_t)b * C + c0) * R + n;
#pragma unroll
  for (int c = 0; c < CH; ++c)
    if (c < nc) dst[(int64_t)c * R] = a[c];
}

// LDS layout of segsum_lds_kernel<T> for (R destinations, NS slots): channels per workgroup and slots per chunk, or false
// when it does not fit
template <typename T>
static bool lds_layout(int64_t B, int64_t C, int64_t R, int64_t NS, int* cpb_out, int* chunk_out) {
  // one chunk: cpb rows of NS slots, state in registers
  int cpb = (int)(SEG_LDS_BYTES / (int64_t)sizeof(T) / (NS > 0 ? NS : 1));
  if (cpb > SEG_CH) cpb = SEG_CH;
  if (cpb >= 1) {
    // enough workgroups to fill the chip when there are many channels
    while (cpb > 1 && B * ((C + cpb - 1) / cpb) < 512) cpb = (cpb + 1) / 2;
    *cpb_out = cpb;
    *chunk_out = (int)NS;
    return true;
  }
  // several chunks, one channel: a row chunk + the running sum (T) and cursor (int) of every destination
  const int64_t chunk = (SEG_LDS_BYTES - R * (int64_t)(sizeof(T) + sizeof(int))) / (int64_t)sizeof(T);
  if (chunk < SEG_MIN_CHUNK) return false;
  *cpb_out = 1;
  *chunk_out = (int)chunk;
  return true;
}

// Which segment-sum kernel takes B scenes, C channels, R destinations and L sources per scene (weighted: L / 3 slots), with
// its channels per workgroup (LDS kernel) or per thread (global kernel) and its slots per chunk: the one place that decides,
// behind segsum() and regnet_scatter_segsum_route.
#define SEG_ROUTE_NONE 0         // no kernel takes the sizes (REGNET_ERR_UNSUPPORTED)
#define SEG_ROUTE_ONE_CHUNK 1    // segsum_lds_kernel, every slot staged at once, state in registers
#define SEG_ROUTE_CHUNKS 2       // segsum_lds_kernel, several chunks, one channel, state in LDS
#define SEG_ROUTE_GLOBAL 3       // segsum_global_kernel
template <typename T>
static int segsum_route(bool weighted, int64_t B, int64_t C, int64_t R, int64_t L, int* kind, int* cpb_out,
                        int* chunk_out) {
  *kind = SEG_ROUTE_NONE;
  *cpb_out = *chunk_out = 0;
  if (!scatter_plan_dims_ok(B, R, L)) return REGNET_ERR_UNSUPPORTED;
  const int64_t NS = weighted ? L / 3 : L;
  int cpb = 0, chunk = 0;
  if (lds_layout<T>(B, C, R, NS, &cpb, &chunk) && (C + cpb - 1) / cpb <= 65535) {
    *kind = NS > chunk ? SEG_ROUTE_CHUNKS : SEG_ROUTE_ONE_CHUNK;
    *cpb_out = cpb;
    *chunk_out = chunk;
    return REGNET_OK;
  }
  if (!seg_g_channels_ok<T>(C) || (R + SEG_G_T - 1) / SEG_G_T >= ((int64_t)1 << 31)) return REGNET_ERR_UNSUPPORTED;
  *kind = SEG_ROUTE_GLOBAL;
  *cpb_out = seg_g_ch<T>;
  return REGNET_OK;
}

extern "C" int regnet_scatter_segsum_route(int elem_size, int weighted, int64_t B, int64_t C, int64_t num_dest,
                                           int64_t num_src, int64_t* route) {
  if (!route) return REGNET_ERR_NULL;
  route[0] = route[1] = route[2] = 0;
  if ((elem_size != 4 && elem_size != 8) || B < 0 || C < 0 || num_dest < 0 || num_src < 0 || (weighted && num_src % 3))
    return REGNET_ERR_SHAPE;
  if (B == 0 || C == 0 || num_dest == 0 || num_src == 0) return REGNET_OK;
  int kind = 0, cpb = 0, chunk = 0;
  const int rc = elem_size == 4 ? segsum_route<float>(weighted != 0, B, C, num_dest, num_src, &kind, &cpb, &chunk)
                                : segsum_route<double>(weighted != 0, B, C, num_dest, num_src, &kind, &cpb, &chunk);
  route[0] = kind;
  route[1] = cpb;
  route[2] = chunk;
  return rc;
}

// gi (B, C, R) = the segment sums of `go` over the plan; REGNET_ERR_UNSUPPORTED when no kernel takes C channels
template <typename T, bool WEIGHTED>
static int segsum(const T* go, int64_t sb, int64_t sc, int64_t s_hi, int64_t s_lo, int64_t inner, const T* weight,
                  int64_t B, int64_t C, int64_t R, int64_t L, const void* plan, T* gi, hipStream_t st) {
  const ScatterPlan pl = scatter_plan_parts(const_cast<void*>(plan), B, R);
  const int64_t NS = WEIGHTED ? L / 3 : L;
  int kind = 0, cpb = 0, chunk = 0;
  const int rc = segsum_route<T>(WEIGHTED, B, C, R, L, &kind, &cpb, &chunk);
  if (rc != REGNET_OK) return rc;
  if (kind != SEG_ROUTE_GLOBAL) {
    static bool attr_set = false;
    if (!attr_set) {
      hipError_t e = hipFuncSetAttribute((const void*)segsum_lds_kernel<T, WEIGHTED>,
                                         hipFuncAttributeMaxDynamicSharedMemorySize, SEG_LDS_BYTES);
      if (e != hipSuccess) return (int)e;
      attr_set = true;
    }
    const bool multi = kind == SEG_ROUTE_CHUNKS;
    const size_t lds = sizeof(T) * ((size_t)cpb * chunk + (multi ? (size_t)cpb * R : 0)) + (multi ? sizeof(int) * R : 0);
    const int dense = !WEIGHTED && s_lo == 1 && s_hi == inner;
    dim3 grid((unsigned)((C + cpb - 1) / cpb), (unsigned)B);
    hipLaunchKernelGGL((segsum_lds_kernel<T, WEIGHTED>), grid, dim3(SEG_T), lds, st, go, sb, sc, s_hi, s_lo, (int)inner,
                       dense, weight, (int)C, (int)R, L, (int)NS, chunk, cpb, pl.off, pl.perm, gi);
    REGNET_LAUNCH_CHECK();
    return REGNET_OK;
  }
  dim3 grid((unsigned)((R + SEG_G_T - 1) / SEG_G_T), (unsigned)((C + seg_g_ch<T> - 1) / seg_g_ch<T>), (unsigned)B);
  hipLaunchKernelGGL((segsum_global_kernel<T, WEIGHTED>), grid, dim3(SEG_G_T), 0, st, go, sb, sc, s_hi, s_lo, (int)inner,
                     weight, (int)C, (int)R, L, pl.off, pl.perm, gi);
  REGNET_LAUNCH_CHECK();
  return REGNET_OK;
}

// =====================================================================================
// Entry points
// =====================================================================================
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
  if (weight) return segsum<float, true>(grad_out, sb, sc, s_hi, 0, 3, weight, B, C, num_dest, num_src, plan, grad_in, st);
  return segsum<float, false>(grad_out, sb, sc, s_hi, s_lo, inner, nullptr, B, C, num_dest, num_src, plan, grad_in, st);
}

extern "C" int64_t regnet_scatter_f64_workspace_bytes(int64_t B, int64_t num_dest, int64_t num_src) {
  return regnet_scatter_plan_bytes(B, num_dest, num_src);   // the workspace holds the plan
}

// float64: the plan of `index` built into the workspace, then the segment sums
template <bool WEIGHTED>
static int scatter_f64(const double* go, int64_t sb, int64_t sc, int64_t s_hi, int64_t s_lo, int64_t inner,
                       const int64_t* index, const double* weight, int64_t B, int64_t C, int64_t R, int64_t L,
                       double* gi, void* workspace, hipStream_t st) {
  if (L == 0) {
    hipError_t e = hipMemsetAsync(gi, 0, sizeof(double) * (size_t)(B * C * R), st);
    return e == hipSuccess ? REGNET_OK : (int)e;
  }
  if (!scatter_plan_dims_ok(B, R, L) || !seg_g_channels_ok<double>(C)) return REGNET_ERR_UNSUPPORTED;
  if (!go || !index || !workspace || (WEIGHTED && !weight)) return REGNET_ERR_NULL;
  const int rc = build_scatter_plan(index, B, R, L, workspace, st);
  if (rc != REGNET_OK) return rc;
  return segsum<double, WEIGHTED>(go, sb, sc, s_hi, s_lo, inner, weight, B, C, R, L, workspace, gi, st);
}

extern "C" int regnet_group_points_bwd_f64(const double* grad_out, int64_t sb, int64_t sc, int64_t sn2, int64_t sk,
                                           const int64_t* index, int64_t B, int64_t C, int64_t N1, int64_t N2,
                                           int64_t K, double* grad_in, void* workspace, void* stream) {
  if (B < 0 || C < 0 || N1 < 0 || N2 < 0 || K < 0) return REGNET_ERR_SHAPE;
  if (B == 0 || C == 0 || N1 == 0) return REGNET_OK;
  if (!grad_in) return REGNET_ERR_NULL;
  if (K >= (int64_t)1 << 31) return REGNET_ERR_UNSUPPORTED;
  return scatter_f64<false>(grad_out, sb, sc, sn2, sk, K, index, nullptr, B, C, N1, N2 * K, grad_in, workspace,
                            as_stream(stream));
}

extern "C" int regnet_gather_knn_bwd_f64(const double* grad_out, int64_t sb, int64_t sc, int64_t sn2, int64_t sk,
                                         const int64_t* index, int64_t B, int64_t C, int64_t N, int64_t NI,
                                         int64_t K, double* grad_in, void* workspace, void* stream) {
  return regnet_group_points_bwd_f64(grad_out, sb, sc, sn2, sk, index, B, C, N, NI, K, grad_in, workspace, stream);
}

extern "C" int regnet_interpolate_bwd_f64(const double* grad_out, int64_t sb, int64_t sc, int64_t sn,
                                          const int64_t* index, const double* weight, int64_t B, int64_t C, int64_t M,
                                          int64_t N, double* grad_in, void* workspace, void* stream) {
  if (B < 0 || C < 0 || M < 0 || N < 0) return REGNET_ERR_SHAPE;
  if (B == 0 || C == 0 || M == 0) return REGNET_OK;
  if (!grad_in) return REGNET_ERR_NULL;
  // source position p = n * 3 + k: row n of grad_out (stride sn), no column stride
  return scatter_f64<true>(grad_out, sb, sc, sn, 0, 3, index, weight, B, C, M, N * 3, grad_in, workspace,
                           as_stream(stream));
}
