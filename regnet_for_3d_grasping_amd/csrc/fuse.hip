// fuse.hip -- voxel-grid merge of up to 8 posed clouds into one cloud on the device (gfx950): one point per occupied voxel, the
// centroid of the voxel's points and colours.  Built with -ffp-contract=off: the pose, the voxel coordinate and its fraction are
// individually rounded float32 operations in the written order, so tests/fuse_reference.py decides every voxel the same way.  No
// float is ever summed: a voxel accumulates integers (24-bit fractions, 8-bit colours), so the result does not depend on the
// order in which the atomics land.  Contract: include/regnet_hip.h, DESIGN.md par. 5.
//
//   stage 1  fuse_accumulate_kernel  a thread per row of ONE view: pose, voxel key, then a slot of the open-addressing table
//                                    (linear probing from a multiplicative hash, claimed by a 64-bit atomicCAS on the key word)
//                                    and nine integer atomics into it.  The row whose count add returned 0 also leaves its
//                                    transformed point and colour in the slot: a voxel of one row is that row, bit for bit.
//   stage 2  fuse_compact_kernel     a thread per slot: the kept voxels' keys and slots compacted in any order
//   (the caller sorts the compacted keys: ascending key order is the output order)
//   stage 3  fuse_emit_kernel        a thread per output row: the slot of rank r, the float64 centroid, the sentinels beyond K
// The probe loop is bounded by the slot count and no thread waits for another: a failed atomicCAS looks at the key it returned
// and moves on.  Key reads are agent-scope atomic loads, so a stale line in a CU's vector cache is never taken for an empty slot.
#include "common.h"

namespace {

constexpr int FUSE_MAX_VIEWS = 8;
constexpr int64_t FUSE_MAX_VOXELS = (int64_t)1 << 21;
constexpr uint64_t FUSE_EMPTY = ~0ull;
constexpr int FUSE_BIAS = 1 << 20;             // voxel coordinates lie in [-2^20, 2^20)
constexpr uint64_t FUSE_HASH = 0x9E3779B97F4A7C15ull;   // 2^64 / golden ratio, odd

struct FuseFrame {   // float32 constants of one view: the pose's first three rows, the origin, 1 / voxel
  float r[12];
  float o[3];
  float inv;
};

struct FuseLayout {   // byte offsets into the workspace
  long long hdr, keys, first, count, views, sum, single, slot_of, total;
};

__host__ inline int64_t fuse_slots(int64_t max_voxels) {
  int64_t p = 1;
  while (p < max_voxels) p <<= 1;
  return 2 * p;
}

__host__ inline FuseLayout fuse_layout(int64_t max_voxels) {
  const long long S = fuse_slots(max_voxels);
  FuseLayout L;
  L.hdr = 0;                        // int32[8]: voxels claimed, rows accumulated, rows dropped, overflow, voxels kept
  L.keys = 64;                      // uint64[S], all ones = empty
  L.first = L.keys + 8 * S;         // uint32[S], all ones = none (keys and first are filled by one memset)
  L.count = L.first + 4 * S;        // int32[S]   (count, views and the sums are zeroed by one memset)
  L.views = L.count + 4 * S;        // int32[S]
  L.sum = L.views + 4 * S;          // uint64[S][6]: S_x, S_y, S_z, C_r, C_g, C_b
  L.single = L.sum + 48 * S;        // float[S][6]: the point and colour of the row that found count == 0
  L.slot_of = L.single + 24 * S;    // int32[max_voxels]: compacted position -> slot
  L.total = (L.slot_of + 4 * max_voxels + 15) / 16 * 16;
  return L;
}

__host__ __device__ inline bool fuse_finite(float v) { return fabsf(v) < __builtin_inff(); }   // (NaN fails)

// Pose, voxel coordinate and fraction of one point, every operation rounded on its own.  false: out of range.
__host__ __device__ inline bool fuse_voxel(float x, float y, float z, const FuseFrame& F, float* p, int* i, float* f) {
  p[0] = affine3(F.r, x, y, z);
  p[1] = affine3(F.r + 4, x, y, z);
  p[2] = affine3(F.r + 8, x, y, z);
  bool ok = true;
#ifdef __HIP_DEVICE_COMPILE__
#pragma unroll
#endif
  for (int k = 0; k < 3; ++k) {
    const float a = (p[k] - F.o[k]) * F.inv;
    const float fl = floorf(a);
    const bool in = fuse_finite(a) && fl >= -1048576.0f && fl < 1048576.0f;
    i[k] = in ? (int)fl : 0;
    f[k] = in ? a - fl : 0.0f;
    ok = ok && in;
  }
  return ok;
}

__host__ __device__ inline uint64_t fuse_key(const int* i) {
  return ((uint64_t)(i[0] + FUSE_BIAS) << 42) | ((uint64_t)(i[1] + FUSE_BIAS) << 21) | (uint64_t)(i[2] + FUSE_BIAS);
}

// the home slot: the top log2(slots) bits of key * FUSE_HASH (mod 2^64); slots is a power of two >= 2
__host__ __device__ inline uint64_t fuse_home(uint64_t key, int log2_slots) { return (key * FUSE_HASH) >> (64 - log2_slots); }

__host__ inline int fuse_log2(int64_t slots) {
  int l = 0;
  while (((int64_t)1 << l) < slots) ++l;
  return l;
}

__device__ __forceinline__ int fuse_colour(float c) {   // (int32)rintf(clamp(c, 0, 1) * 255.0f); NaN counts as 0
  if (!(c > 0.0f)) return 0;
  return (int)rintf(fminf(c, 1.0f) * 255.0f);
}

// wave-aggregated counter: one atomicAdd per wave for the lanes whose `flag` is set
__device__ __forceinline__ void fuse_tally(bool flag, int* counter) {
  const uint64_t votes = __ballot(flag);
  if (votes != 0ull && lane_id() == __builtin_ctzll(votes)) atomicAdd(counter, (int)__popcll(votes));
}

__global__ __launch_bounds__(256) void fuse_accumulate_kernel(const float* __restrict__ xyz, const float* __restrict__ rgb, int n,
                                                              int view, int row_offset, FuseFrame F, int max_voxels,
                                                              unsigned slot_mask, int log2_slots, int* __restrict__ hdr,
                                                              unsigned long long* __restrict__ keys,
                                                              unsigned* __restrict__ first, int* __restrict__ count,
                                                              int* __restrict__ views, unsigned long long* __restrict__ sum,
                                                              float* __restrict__ single) {
  const int r = blockIdx.x * 256 + threadIdx.x;
  bool finite = false, inside = false;
  float p[3], f[3];
  int i[3];
  if (r < n) {
    const float x = xyz[(int64_t)r * 3], y = xyz[(int64_t)r * 3 + 1], z = xyz[(int64_t)r * 3 + 2];
    finite = fuse_finite(x) && fuse_finite(y) && fuse_finite(z);
    inside = finite && fuse_voxel(x, y, z, F, p, i, f);
  }
  int slot = -1;
  bool overflow = false;
  if (inside) {
    const uint64_t key = fuse_key(i);
    unsigned s = (unsigned)fuse_home(key, log2_slots);
    for (unsigned probe = 0; probe <= slot_mask; ++probe, s = (s + 1u) & slot_mask) {
      uint64_t cur = __hip_atomic_load(&keys[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (cur == FUSE_EMPTY) {
        cur = atomicCAS(&keys[s], (unsigned long long)FUSE_EMPTY, (unsigned long long)key);
        if (cur == FUSE_EMPTY) {                       // this row opened the voxel: is it one of the first max_voxels?
          if (atomicAdd(&hdr[0], 1) < max_voxels) slot = (int)s; else overflow = true;
          break;
        }
      }
      if (cur == key) { slot = (int)s; break; }
    }
    overflow = overflow || slot < 0;                   // (or the table holds no free slot on this row's probe path)
  }
  if (slot >= 0) {
    float c[3] = {0.0f, 0.0f, 0.0f};
    if (rgb != nullptr) { c[0] = rgb[(int64_t)r * 3]; c[1] = rgb[(int64_t)r * 3 + 1]; c[2] = rgb[(int64_t)r * 3 + 2]; }
    unsigned long long* acc = sum + (int64_t)slot * 6;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      atomicAdd(&acc[k], (unsigned long long)(int)(f[k] * 16777216.0f));
      atomicAdd(&acc[3 + k], (unsigned long long)fuse_colour(c[k]));
    }
    atomicMin(&first[slot], (unsigned)(row_offset + r));
    atomicOr(&views[slot], 1 << view);
    if (atomicAdd(&count[slot], 1) == 0) {             // exactly one row of a voxel sees 0; read only when the count stays 1
      float* one = single + (int64_t)slot * 6;
#pragma unroll
      for (int k = 0; k < 3; ++k) { one[k] = p[k]; one[3 + k] = c[k]; }
    }
  }
  fuse_tally(slot >= 0, &hdr[1]);
  fuse_tally(r < n && !inside, &hdr[2]);
  if (overflow) hdr[3] = 1;
}

__global__ __launch_bounds__(256) void fuse_fill_kernel(long long* __restrict__ kept_keys, int max_voxels, int* __restrict__ hdr) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t < max_voxels) kept_keys[t] = 0x7fffffffffffffffll;   // above every key: the unused tail sorts last
  if (t == 0) hdr[4] = 0;
}

__global__ __launch_bounds__(256) void fuse_compact_kernel(const unsigned long long* __restrict__ keys,
                                                           const int* __restrict__ count, unsigned slots, int min_count,
                                                           int max_voxels, int* __restrict__ hdr,
                                                           long long* __restrict__ kept_keys, int* __restrict__ slot_of) {
  const unsigned s = blockIdx.x * 256u + threadIdx.x;
  const bool kept = s < slots && keys[s] != FUSE_EMPTY && count[s] >= min_count;
  const int pos = wave_append(kept, &hdr[4]);
  if (kept) {
    if (pos < max_voxels) {
      kept_keys[pos] = (long long)keys[s];
      slot_of[pos] = (int)s;
    } else {
      hdr[3] = 1;
    }
  }
}

__global__ __launch_bounds__(256) void fuse_emit_kernel(const long long* __restrict__ order, const int* __restrict__ slot_of,
                                                        const unsigned long long* __restrict__ keys,
                                                        const unsigned* __restrict__ first, const int* __restrict__ count,
                                                        const int* __restrict__ views,
                                                        const unsigned long long* __restrict__ sum,
                                                        const float* __restrict__ single, const int* __restrict__ hdr,
                                                        unsigned slots, int max_voxels, float ox, float oy, float oz, float inv,
                                                        float* __restrict__ out_xyz, float* __restrict__ out_rgb,
                                                        int* __restrict__ out_count, int* __restrict__ out_views,
                                                        int* __restrict__ out_first, int* __restrict__ num) {
  const int r = blockIdx.x * 256 + threadIdx.x;
  const int K = min(hdr[4], max_voxels);
  if (r == 0) {
    num[0] = K;
    num[1] = hdr[1];
    num[2] = hdr[2];
    num[3] = (hdr[3] != 0 || hdr[4] > max_voxels) ? 1 : 0;
  }
  if (r >= max_voxels) return;
  float xyz[3] = {__uint_as_float(0x7fc00000u), __uint_as_float(0x7fc00000u), __uint_as_float(0x7fc00000u)};
  float rgb[3] = {0.0f, 0.0f, 0.0f};
  int n = -1, v = -1, fr = -1;
  if (r < K) {
    const long long pos = order[r];
    const int s = (pos >= 0 && pos < max_voxels) ? slot_of[pos] : -1;
    if (s >= 0 && (unsigned)s < slots) {
      n = count[s];
      v = views[s];
      fr = (int)first[s];
      if (n == 1) {
#pragma unroll
        for (int k = 0; k < 3; ++k) { xyz[k] = single[(int64_t)s * 6 + k]; rgb[k] = single[(int64_t)s * 6 + 3 + k]; }
      } else {
        const uint64_t key = keys[s];
        const int i[3] = {(int)((key >> 42) & 0x1fffffu) - FUSE_BIAS, (int)((key >> 21) & 0x1fffffu) - FUSE_BIAS,
                          (int)(key & 0x1fffffu) - FUSE_BIAS};
        const float o[3] = {ox, oy, oz};
        const double cells = (double)n * 16777216.0, levels = (double)n * 255.0;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
          const double a_mean = (double)i[k] + (double)(long long)sum[(int64_t)s * 6 + k] / cells;
          xyz[k] = (float)((double)o[k] + a_mean / (double)inv);
          rgb[k] = (float)((double)(long long)sum[(int64_t)s * 6 + 3 + k] / levels);
        }
      }
    }
  }
#pragma unroll
  for (int k = 0; k < 3; ++k) { out_xyz[(int64_t)r * 3 + k] = xyz[k]; out_rgb[(int64_t)r * 3 + k] = rgb[k]; }
  out_count[r] = n;
  out_views[r] = v;
  out_first[r] = fr;
}

__host__ inline bool fuse_voxel_ok(double voxel) { return voxel > 0.0 && voxel < __builtin_inf(); }

__host__ inline FuseFrame fuse_frame(const float* pose12, const float* origin3, float inv) {
  FuseFrame F;
  for (int k = 0; k < 12; ++k) F.r[k] = pose12[k];
  for (int k = 0; k < 3; ++k) F.o[k] = origin3[k];
  F.inv = inv;
  return F;
}

}  // namespace

extern "C" int64_t regnet_fuse_table_slots(int64_t max_voxels) {
  if (max_voxels < 1 || max_voxels > FUSE_MAX_VOXELS) return -1;
  return fuse_slots(max_voxels);
}

extern "C" int64_t regnet_fuse_workspace_bytes(int64_t max_voxels) {
  if (max_voxels < 1 || max_voxels > FUSE_MAX_VOXELS) return -1;
  return fuse_layout(max_voxels).total;
}

extern "C" int regnet_fuse_key_host(float x, float y, float z, const float* pose12, const float* origin3, float inv,
                                    uint64_t* key) {
  if (!pose12 || !origin3 || !key) return REGNET_ERR_NULL;
  float p[3], f[3];
  int i[3];
  *key = FUSE_EMPTY;
  if (!(fuse_finite(x) && fuse_finite(y) && fuse_finite(z))) return 1;
  if (!fuse_voxel(x, y, z, fuse_frame(pose12, origin3, inv), p, i, f)) return 2;
  *key = fuse_key(i);
  return REGNET_OK;
}

extern "C" int64_t regnet_fuse_home_slot_host(uint64_t key, int64_t slots) {
  if (slots < 2 || slots > 2 * FUSE_MAX_VOXELS || (slots & (slots - 1)) != 0) return -1;
  return (int64_t)fuse_home(key, fuse_log2(slots));
}

extern "C" int regnet_fuse_accumulate_f32(const float* xyz, const float* rgb, int64_t n, int view, int64_t row_offset,
                                          const float* pose12, const float* origin3, double voxel, int64_t max_voxels,
                                          int reset, void* workspace, void* stream) {
  if (n < 0 || row_offset < 0 || view < 0) return REGNET_ERR_SHAPE;
  if (view >= FUSE_MAX_VIEWS || !fuse_voxel_ok(voxel) || max_voxels < 1 || max_voxels > FUSE_MAX_VOXELS ||
      row_offset + n >= (int64_t)1 << 31)
    return REGNET_ERR_UNSUPPORTED;
  if (!workspace || !pose12 || !origin3 || (n > 0 && !xyz)) return REGNET_ERR_NULL;
  hipStream_t st = as_stream(stream);
  const FuseLayout L = fuse_layout(max_voxels);
  const int64_t S = fuse_slots(max_voxels);
  char* ws = (char*)workspace;
  if (reset) {
    hipError_t e = hipMemsetAsync(ws + L.hdr, 0, 64, st);
    if (e == hipSuccess) e = hipMemsetAsync(ws + L.keys, 0xff, (size_t)(12 * S), st);
    if (e == hipSuccess) e = hipMemsetAsync(ws + L.count, 0, (size_t)(56 * S), st);
    if (e != hipSuccess) return (int)e;
  }
  if (n == 0) return REGNET_OK;
  const FuseFrame F = fuse_frame(pose12, origin3, (float)(1.0 / voxel));
  hipLaunchKernelGGL(fuse_accumulate_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, xyz, rgb, (int)n, view,
                     (int)row_offset, F, (int)max_voxels, (unsigned)(S - 1), fuse_log2(S), (int*)(ws + L.hdr),
                     (unsigned long long*)(ws + L.keys), (unsigned*)(ws + L.first), (int*)(ws + L.count),
                     (int*)(ws + L.views), (unsigned long long*)(ws + L.sum), (float*)(ws + L.single));
  REGNET_LAUNCH_CHECK();
  return REGNET_OK;
}

extern "C" int regnet_fuse_finalise_f32(int64_t max_voxels, int64_t min_count, int64_t* kept_keys, void* workspace,
                                        void* stream) {
  if (min_count < 1) return REGNET_ERR_SHAPE;
  if (max_voxels < 1 || max_voxels > FUSE_MAX_VOXELS) return REGNET_ERR_UNSUPPORTED;
  if (!workspace || !kept_keys) return REGNET_ERR_NULL;
  hipStream_t st = as_stream(stream);
  const FuseLayout L = fuse_layout(max_voxels);
  const int64_t S = fuse_slots(max_voxels);
  char* ws = (char*)workspace;
  const int mc = (int)(min_count > 0x7fffffff ? 0x7fffffff : min_count);
  hipLaunchKernelGGL(fuse_fill_kernel, dim3((unsigned)((max_voxels + 255) / 256)), dim3(256), 0, st, (long long*)kept_keys,
                     (int)max_voxels, (int*)(ws + L.hdr));
  hipLaunchKernelGGL(fuse_compact_kernel, dim3((unsigned)((S + 255) / 256)), dim3(256), 0, st,
                     (const unsigned long long*)(ws + L.keys), (const int*)(ws + L.count), (unsigned)S, mc, (int)max_voxels,
                     (int*)(ws + L.hdr), (long long*)kept_keys, (int*)(ws + L.slot_of));
  REGNET_LAUNCH_CHECK();
  return REGNET_OK;
}

extern "C" int regnet_fuse_emit_f32(const int64_t* order, const float* origin3, double voxel, int64_t max_voxels, float* xyz,
                                    float* rgb, int32_t* count, int32_t* views, int32_t* first, int32_t* num, void* workspace,
                                    void* stream) {
  if (max_voxels < 1 || max_voxels > FUSE_MAX_VOXELS || !fuse_voxel_ok(voxel)) return REGNET_ERR_UNSUPPORTED;
  if (!workspace || !order || !origin3 || !xyz || !rgb || !count || !views || !first || !num) return REGNET_ERR_NULL;
  const FuseLayout L = fuse_layout(max_voxels);
  const int64_t S = fuse_slots(max_voxels);
  char* ws = (char*)workspace;
  hipLaunchKernelGGL(fuse_emit_kernel, dim3((unsigned)((max_voxels + 255) / 256)), dim3(256), 0, as_stream(stream),
                     (const long long*)order, (const int*)(ws + L.slot_of), (const unsigned long long*)(ws + L.keys),
                     (const unsigned*)(ws + L.first), (const int*)(ws + L.count), (const int*)(ws + L.views),
                     (const unsigned long long*)(ws + L.sum), (const float*)(ws + L.single), (const int*)(ws + L.hdr),
                     (unsigned)S, (int)max_voxels, origin3[0], origin3[1], origin3[2], (float)(1.0 / voxel), xyz, rgb,
                     (int*)count, (int*)views, (int*)first, (int*)num);
  REGNET_LAUNCH_CHECK();
  return REGNET_OK;
}
