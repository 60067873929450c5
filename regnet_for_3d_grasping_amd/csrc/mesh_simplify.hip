// mesh_simplify.hip -- vertex clustering of a triangle mesh on the device (gfx950): the vertices of a Surface are merged per cell of
// a dense coarse grid, the index buffer of a Mesh is remapped, collapsed triangles leave and equal ones are made one.
//
// The contract is include/regnet_hip.h "Mesh simplification" and DESIGN.md par. 5.  Integer accumulation only (fuse.hip's voxel
// merge applied to vertices), the order of the grid is the order of the output, and of equal triangles the smallest source row
// survives (atomicMin): the bytes do not depend on the order in which threads arrive, and tests/mesh_simplify_reference.py
// restates them with plain loops.  Built with -ffp-contract=off: the cell arithmetic and the float64 finalise are individually
// rounded operations in the written order.
//
//   two memsets            the cells' sums and counters to 0, the triangle set's keys and rows and the cells' first row to all ones
//   ms_vertex_kernel       a thread per vertex row < K: its cell, then integer atomics into the cell (count, S, C, N, ncount, first)
//   ms_insert_kernel       a thread per source triangle < Kt: ABSENT / STRAY / COLLAPSED, or the key of its canonical rotation; with
//                          dedupe the key goes into the open-addressing set (fuse.hip's probe loop) and atomicMin leaves the smallest
//                          source row in the slot
//   ms_survive_kernel      a thread per source triangle: it survives when it holds its slot's row; a survivor marks its three cells
//                          as referenced (a plain store of 1) -- and the survivors per block of 256 source rows
//   ms_cell_count_kernel   a thread per cell: the referenced cells per block of 256 cells, the occupied cells
//   ms_scan_kernel         ONE workgroup turns both arrays of block counts into exclusive bases (at most 16 blocks per thread)
//   ms_vertex_emit_kernel  a thread per cell: the new row of a referenced cell (block base + ballot rank), left in place of the
//                          mark, and the finalised vertex when the row is below max_vertices
//   ms_tri_emit_kernel     a thread per source triangle: a survivor's output row (block base + ballot rank) receives the new rows of
//                          its three cells, or (-1, -1, -1) when one of them is beyond max_vertices
//   ms_tail_kernel         the sentinel rows beyond the kept counts, num and surface_num
// The launches are ordered by the stream: no thread waits for another, every probe loop ends on the slot count, no cooperative
// launch, no sort, no host read, no allocation.
#include "common.h"

namespace {

constexpr int64_t MS_MAX_CELLS = (int64_t)1 << 21;
constexpr int64_t MS_MAX_VERTICES = (int64_t)1 << 21;
constexpr int64_t MS_MAX_TRIANGLES = (int64_t)1 << 22;
constexpr int MS_BLOCK = 256;
constexpr int MS_WAVES = MS_BLOCK / 64;
constexpr int MS_SCAN = 1024;                                   // threads of the one scanning workgroup
constexpr uint64_t MS_EMPTY = ~0ull;                            // no key: a key has 63 bits
constexpr uint64_t MS_HASH = 0x9E3779B97F4A7C15ull;             // fuse.hip's FUSE_HASH: 2^64 / golden ratio, odd
constexpr unsigned MS_QNAN = 0x7fc00000u;

// hdr words
enum { H_OCCUPIED = 0, H_STRAY_V, H_COLLAPSED, H_DUPLICATE, H_STRAY_T, H_DROPPED, H_KV, H_SURVIVORS, H_WORDS = 16 };

struct MsLayout {   // byte offsets into the workspace
  long long hdr, sums, count, ncount, mark, zero_end;           // zeroed by one memset
  long long keys, min_row, first, ones_end;                     // set to all ones by one memset
  long long tri_key, tri_slot, cell_blocks, tri_blocks, total;  // written before they are read
};

__host__ inline int64_t ms_slots(int64_t max_tri_in) {
  int64_t p = 1;
  while (p < max_tri_in) p <<= 1;
  return 2 * p;
}

__host__ inline int ms_log2(int64_t slots) {
  int l = 0;
  while (((int64_t)1 << l) < slots) ++l;
  return l;
}

// the home slot, fuse.hip's: the top log2(slots) bits of key * MS_HASH (mod 2^64); slots is a power of two >= 2
__host__ __device__ inline uint64_t ms_home(uint64_t key, int log2_slots) { return (key * MS_HASH) >> (64 - log2_slots); }

__host__ inline int64_t ms_blocks(int64_t n) { return (n + MS_BLOCK - 1) / MS_BLOCK; }

__host__ inline MsLayout ms_layout(int64_t G, int64_t max_tri_in) {
  const long long S = ms_slots(max_tri_in);
  MsLayout L;
  L.hdr = 0;                                      // int32[16]
  L.sums = 64;                                    // int64[G][9]: S_xyz, C_rgb, N_xyz
  L.count = L.sums + 72 * G;                      // int32[G]
  L.ncount = L.count + 4 * G;                     // int32[G]
  L.mark = L.ncount + 4 * G;                      // int32[G]: referenced by a survivor; then the new row, -1 without one
  L.zero_end = (L.mark + 4 * G + 7) / 8 * 8;
  L.keys = L.zero_end;                            // uint64[S]
  L.min_row = L.keys + 8 * S;                     // uint32[S]
  L.first = L.min_row + 4 * S;                    // uint32[G]
  L.ones_end = (L.first + 4 * G + 7) / 8 * 8;
  L.tri_key = L.ones_end;                         // uint64[max_tri_in]: the key of a row that may survive, else all ones
  L.tri_slot = L.tri_key + 8 * max_tri_in;        // int32[max_tri_in]
  L.cell_blocks = L.tri_slot + 4 * max_tri_in;    // int32[blocks of cells]: counts, then exclusive bases
  L.tri_blocks = L.cell_blocks + 4 * ms_blocks(G);
  L.total = (L.tri_blocks + 4 * ms_blocks(max_tri_in) + 15) / 16 * 16;
  return L;
}

struct MsGrid {
  float o[3];
  float cell;
  int g[3];
  int G;
};

__device__ __forceinline__ bool ms_finite(float v) { return fabsf(v) < __builtin_inff(); }   // (NaN fails)

// the cell of a vertex and its fractions; -1: a STRAY vertex
__device__ __forceinline__ int ms_cell(const float* __restrict__ xyz, int r, const MsGrid& grid, float* f) {
  int i[3];
  bool ok = true;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const float x = xyz[(int64_t)r * 3 + k];
    const float a = __fdiv_rn(x - grid.o[k], grid.cell);
    const float fl = floorf(a);
    const bool in = ms_finite(x) && fl >= 0.0f && fl < (float)grid.g[k];      // (a NaN or infinite quotient fails)
    i[k] = in ? (int)fl : 0;
    f[k] = in ? a - (float)i[k] : 0.0f;
    ok = ok && in;
  }
  return ok ? (i[2] * grid.g[1] + i[1]) * grid.g[0] + i[0] : -1;
}

__device__ __forceinline__ int ms_colour(float c) {   // (int32)rintf(clamp(c, 0, 1) * 255.0f); NaN counts as 0
  if (!(c > 0.0f)) return 0;
  return (int)rintf(fminf(c, 1.0f) * 255.0f);
}

// wave-aggregated counter: one atomicAdd per wave for the lanes whose `flag` is set
__device__ __forceinline__ void ms_tally(bool flag, int* counter) {
  const uint64_t votes = __ballot(flag);
  if (votes != 0ull && lane_id() == __builtin_ctzll(votes)) atomicAdd(counter, (int)__popcll(votes));
}

// the rank of this thread among the flagged threads of its workgroup, in thread order; every thread of the workgroup calls it
// -> (rank, the workgroup's total)
__device__ __forceinline__ int ms_block_rank(bool flag, int* s_total, int& total) {
  const uint64_t votes = __ballot(flag);
  const int wave = threadIdx.x >> 6;
  if (lane_id() == 0) s_total[wave] = (int)__popcll(votes);
  __syncthreads();
  int rank = mbcnt64(votes);
  total = 0;
#pragma unroll
  for (int w = 0; w < MS_WAVES; ++w) {
    if (w < wave) rank += s_total[w];
    total += s_total[w];
  }
  return rank;
}

__global__ __launch_bounds__(MS_BLOCK) void ms_vertex_kernel(const float* __restrict__ xyz, const float* __restrict__ normal,
                                                             const float* __restrict__ rgb, const int32_t* __restrict__ K_source,
                                                             int rows, MsGrid grid, int* __restrict__ hdr,
                                                             unsigned long long* __restrict__ sums, int* __restrict__ count,
                                                             int* __restrict__ ncount, unsigned* __restrict__ first) {
  const int r = blockIdx.x * MS_BLOCK + threadIdx.x;
  const int K = min(max(K_source[0], 0), rows);
  float f[3];
  const int c = r < K ? ms_cell(xyz, r, grid, f) : -1;
  ms_tally(r < K && c < 0, &hdr[H_STRAY_V]);
  if (c < 0) return;
  unsigned long long* acc = sums + (int64_t)c * 9;
  float n[3];
  bool with_normal = true;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    atomicAdd(&acc[k], (unsigned long long)(long long)(int)(f[k] * 16777216.0f));
    atomicAdd(&acc[3 + k], (unsigned long long)(long long)ms_colour(rgb[(int64_t)r * 3 + k]));
    n[k] = normal[(int64_t)r * 3 + k];
    with_normal = with_normal && ms_finite(n[k]);
  }
  if (with_normal) {
#pragma unroll
    for (int k = 0; k < 3; ++k)
      atomicAdd(&acc[6 + k], (unsigned long long)(long long)(int)rintf(fminf(fmaxf(n[k], -1.0f), 1.0f) * 1048576.0f));
    atomicAdd(&ncount[c], 1);
  }
  atomicMin(&first[c], (unsigned)r);
  atomicAdd(&count[c], 1);
}

__global__ __launch_bounds__(MS_BLOCK) void ms_insert_kernel(const float* __restrict__ xyz, const int32_t* __restrict__ K_source,
                                                             int rows, const int32_t* __restrict__ tri,
                                                             const int32_t* __restrict__ num_tri_in, int max_tri_in, MsGrid grid,
                                                             int dedupe, unsigned slot_mask, int log2_slots, int* __restrict__ hdr,
                                                             unsigned long long* __restrict__ keys, unsigned* __restrict__ min_row,
                                                             unsigned long long* __restrict__ tri_key,
                                                             int* __restrict__ tri_slot) {
  const int t = blockIdx.x * MS_BLOCK + threadIdx.x;
  const int K = min(max(K_source[0], 0), rows);
  const int Kt = min(max(num_tri_in[0], 0), max_tri_in);
  bool stray = false, collapsed = false;
  uint64_t key = MS_EMPTY;
  if (t < Kt) {
    const int v[3] = {tri[(int64_t)t * 3], tri[(int64_t)t * 3 + 1], tri[(int64_t)t * 3 + 2]};
    int c[3] = {-1, -1, -1};
    stray = true;                                     // (ABSENT rows are counted with the STRAY ones)
    if (v[0] >= 0 && v[0] < K && v[1] >= 0 && v[1] < K && v[2] >= 0 && v[2] < K) {
      float f[3];
#pragma unroll
      for (int k = 0; k < 3; ++k) c[k] = ms_cell(xyz, v[k], grid, f);
      stray = c[0] < 0 || c[1] < 0 || c[2] < 0;
    }
    if (!stray) {
      collapsed = c[0] == c[1] || c[1] == c[2] || c[2] == c[0];
      if (!collapsed) {                               // the cyclic rotation with the smallest cell first
        const int lo = (c[0] < c[1] && c[0] < c[2]) ? 0 : (c[1] < c[2] ? 1 : 2);
        key = ((uint64_t)c[lo] << 42) | ((uint64_t)c[(lo + 1) % 3] << 21) | (uint64_t)c[(lo + 2) % 3];
      }
    }
  }
  ms_tally(stray, &hdr[H_STRAY_T]);
  ms_tally(collapsed, &hdr[H_COLLAPSED]);
  if (t >= Kt) return;
  int slot = -1;
  if (key != MS_EMPTY && dedupe) {
    unsigned s = (unsigned)ms_home(key, log2_slots);
    for (unsigned probe = 0; probe <= slot_mask; ++probe, s = (s + 1u) & slot_mask) {
      uint64_t cur = __hip_atomic_load(&keys[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (cur == MS_EMPTY) cur = atomicCAS(&keys[s], (unsigned long long)MS_EMPTY, (unsigned long long)key);
      if (cur == MS_EMPTY || cur == key) { slot = (int)s; break; }
    }
    if (slot >= 0) atomicMin(&min_row[slot], (unsigned)t);      // (the table has twice max_tri_in slots: it cannot fill)
  }
  tri_key[t] = key;
  tri_slot[t] = slot;
}

__global__ __launch_bounds__(MS_BLOCK) void ms_survive_kernel(const int32_t* __restrict__ num_tri_in, int max_tri_in, int dedupe,
                                                              int G, const unsigned* __restrict__ min_row,
                                                              unsigned long long* __restrict__ tri_key,
                                                              const int* __restrict__ tri_slot, int* __restrict__ mark,
                                                              int* __restrict__ hdr, int* __restrict__ tri_blocks) {
  __shared__ int s_total[MS_WAVES];
  const int t = blockIdx.x * MS_BLOCK + threadIdx.x;
  const int Kt = min(max(num_tri_in[0], 0), max_tri_in);
  bool survives = false, duplicate = false;
  if (t < Kt) {
    const uint64_t key = tri_key[t];
    if (key != MS_EMPTY) {
      const int slot = tri_slot[t];
      survives = !dedupe || (slot >= 0 && min_row[slot] == (unsigned)t);
      duplicate = !survives;
      if (duplicate) tri_key[t] = MS_EMPTY;
      if (survives) {
        const int c[3] = {(int)(key >> 42), (int)((key >> 21) & 0x1fffffu), (int)(key & 0x1fffffu)};
#pragma unroll
        for (int k = 0; k < 3; ++k)
          if (c[k] < G) mark[c[k]] = 1;                // (every writer stores the same word)
      }
    }
  }
  ms_tally(duplicate, &hdr[H_DUPLICATE]);
  int total;
  ms_block_rank(survives, s_total, total);
  if (threadIdx.x == 0) tri_blocks[blockIdx.x] = total;
}

__global__ __launch_bounds__(MS_BLOCK) void ms_cell_count_kernel(const int* __restrict__ mark, const int* __restrict__ count, int G,
                                                                 int* __restrict__ hdr, int* __restrict__ cell_blocks) {
  __shared__ int s_total[MS_WAVES];
  const int c = blockIdx.x * MS_BLOCK + threadIdx.x;
  ms_tally(c < G && count[c] > 0, &hdr[H_OCCUPIED]);
  int total;
  ms_block_rank(c < G && mark[c] != 0, s_total, total);
  if (threadIdx.x == 0) cell_blocks[blockIdx.x] = total;
}

// counts[0 .. n) -> its exclusive prefix sums in place, the total to *total_out; one workgroup of MS_SCAN threads, every thread
// of which calls it: thread i owns the `per` consecutive entries from i * per
__device__ __forceinline__ void ms_scan(int* __restrict__ counts, int n, int* __restrict__ total_out, int* s_wave) {
  const int per = (n + MS_SCAN - 1) / MS_SCAN;
  const int begin = min((int)threadIdx.x * per, n), end = min(begin + per, n);
  int mine = 0;
  for (int j = begin; j < end; ++j) mine += counts[j];
  int incl = mine;                                    // the inclusive scan of a wave: 6 shuffles
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int up = __shfl_up(incl, o);
    if (lane_id() >= o) incl += up;
  }
  const int wave = threadIdx.x >> 6;
  if (lane_id() == 63) s_wave[wave] = incl;
  __syncthreads();
  int base = incl - mine, total = 0;
  for (int w = 0; w < MS_SCAN / 64; ++w) {
    if (w < wave) base += s_wave[w];
    total += s_wave[w];
  }
  for (int j = begin; j < end; ++j) {
    const int v = counts[j];
    counts[j] = base;
    base += v;
  }
  if (threadIdx.x == 0) *total_out = total;
  __syncthreads();                                    // (s_wave is free again)
}

__global__ __launch_bounds__(MS_SCAN) void ms_scan_kernel(int* __restrict__ cell_blocks, int n_cell_blocks,
                                                          int* __restrict__ tri_blocks, int n_tri_blocks, int* __restrict__ hdr) {
  __shared__ int s_wave[MS_SCAN / 64];
  ms_scan(cell_blocks, n_cell_blocks, &hdr[H_KV], s_wave);
  ms_scan(tri_blocks, n_tri_blocks, &hdr[H_SURVIVORS], s_wave);
}

__global__ __launch_bounds__(MS_BLOCK) void ms_vertex_emit_kernel(const float* __restrict__ xyz, const float* __restrict__ normal,
                                                                  const float* __restrict__ rgb, MsGrid grid,
                                                                  const unsigned long long* __restrict__ sums,
                                                                  const int* __restrict__ count, const int* __restrict__ ncount,
                                                                  const unsigned* __restrict__ first, int* __restrict__ mark,
                                                                  const int* __restrict__ cell_blocks, int max_vertices,
                                                                  float* __restrict__ out_xyz, float* __restrict__ out_normal,
                                                                  float* __restrict__ out_rgb, int32_t* __restrict__ out_weight) {
  __shared__ int s_total[MS_WAVES];
  const int c = blockIdx.x * MS_BLOCK + threadIdx.x;
  const bool kept = c < grid.G && mark[c] != 0;
  int total;
  const int row = cell_blocks[blockIdx.x] + ms_block_rank(kept, s_total, total);
  if (c < grid.G) mark[c] = kept ? row : -1;
  if (!kept || row >= max_vertices) return;
  const int n = count[c];
  float p[3], q[3], col[3];
  if (n == 1) {                                       // the one row of the cell as it was given, bit for bit
    const int64_t r = (int64_t)first[c];
#pragma unroll
    for (int k = 0; k < 3; ++k) { p[k] = xyz[r * 3 + k]; q[k] = normal[r * 3 + k]; col[k] = rgb[r * 3 + k]; }
  } else {
    const int i[3] = {c % grid.g[0], c / grid.g[0] % grid.g[1], c / grid.g[0] / grid.g[1]};
    const long long* acc = (const long long*)sums + (int64_t)c * 9;
    const double cells = (double)n * 16777216.0, levels = (double)n * 255.0;
    double m[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const double a_mean = (double)i[k] + (double)acc[k] / cells;
      p[k] = (float)((double)grid.o[k] + a_mean * (double)grid.cell);
      col[k] = (float)((double)acc[3 + k] / levels);
      m[k] = (double)acc[6 + k] / 1048576.0;
    }
    const double len = sqrt((m[0] * m[0] + m[1] * m[1]) + m[2] * m[2]);
    const bool with_normal = ncount[c] != 0 && len != 0.0;
#pragma unroll
    for (int k = 0; k < 3; ++k) q[k] = with_normal ? (float)(m[k] / len) : __uint_as_float(MS_QNAN);
  }
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    out_xyz[(int64_t)row * 3 + k] = p[k];
    out_normal[(int64_t)row * 3 + k] = q[k];
    out_rgb[(int64_t)row * 3 + k] = col[k];
  }
  out_weight[row] = n;
}

__global__ __launch_bounds__(MS_BLOCK) void ms_tri_emit_kernel(const int32_t* __restrict__ num_tri_in, int max_tri_in, int G,
                                                               const unsigned long long* __restrict__ tri_key,
                                                               const int* __restrict__ mark, const int* __restrict__ tri_blocks,
                                                               int max_vertices, int max_triangles, int32_t* __restrict__ out_tri,
                                                               int* __restrict__ hdr) {
  __shared__ int s_total[MS_WAVES];
  const int t = blockIdx.x * MS_BLOCK + threadIdx.x;
  const int Kt = min(max(num_tri_in[0], 0), max_tri_in);
  const uint64_t key = t < Kt ? tri_key[t] : MS_EMPTY;
  const bool survives = key != MS_EMPTY;
  int total;
  const int row = tri_blocks[blockIdx.x] + ms_block_rank(survives, s_total, total);
  bool dropped = false;
  if (survives && row < max_triangles) {
    const int c[3] = {(int)(key >> 42), (int)((key >> 21) & 0x1fffffu), (int)(key & 0x1fffffu)};
    int v[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      v[k] = c[k] < G ? mark[c[k]] : -1;
      dropped = dropped || v[k] < 0 || v[k] >= max_vertices;
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) out_tri[(int64_t)row * 3 + k] = dropped ? -1 : v[k];
  }
  ms_tally(dropped, &hdr[H_DROPPED]);
}

__global__ __launch_bounds__(MS_BLOCK) void ms_tail_kernel(const int* __restrict__ hdr, const int32_t* __restrict__ K_source,
                                                           int rows, int max_vertices, int max_triangles,
                                                           float* __restrict__ out_xyz, float* __restrict__ out_normal,
                                                           float* __restrict__ out_rgb, int32_t* __restrict__ out_weight,
                                                           int32_t* __restrict__ out_tri, int32_t* __restrict__ num,
                                                           int32_t* __restrict__ surface_num) {
  const int Kv_all = hdr[H_KV], Kv = min(Kv_all, max_vertices);
  const int Kt_all = hdr[H_SURVIVORS], Kt = min(Kt_all, max_triangles);
  const int r = blockIdx.x * MS_BLOCK + threadIdx.x;
  if (r == 0) {
    num[0] = Kv; num[1] = Kv_all; num[2] = Kv_all > max_vertices ? 1 : 0;
    num[3] = hdr[H_OCCUPIED]; num[4] = hdr[H_STRAY_V];
    num[5] = Kt; num[6] = Kt_all; num[7] = hdr[H_DROPPED]; num[8] = Kt_all > max_triangles ? 1 : 0;
    num[9] = hdr[H_COLLAPSED]; num[10] = hdr[H_DUPLICATE]; num[11] = hdr[H_STRAY_T];
    if (surface_num != nullptr) {
      surface_num[0] = Kv; surface_num[1] = Kv_all; surface_num[2] = min(max(K_source[0], 0), rows);
      surface_num[3] = Kv_all > max_vertices ? 1 : 0;
    }
  }
  if (r >= Kv && r < max_vertices) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      out_xyz[(int64_t)r * 3 + k] = __uint_as_float(MS_QNAN);
      out_normal[(int64_t)r * 3 + k] = __uint_as_float(MS_QNAN);
      out_rgb[(int64_t)r * 3 + k] = 0.0f;
    }
    out_weight[r] = -1;
  }
  if (r >= Kt && r < max_triangles) {
#pragma unroll
    for (int k = 0; k < 3; ++k) out_tri[(int64_t)r * 3 + k] = -1;
  }
}

int ms_sizes(int64_t G, int64_t max_tri_in) {
  if (G < 1 || max_tri_in < 1) return REGNET_ERR_SHAPE;
  if (G > MS_MAX_CELLS || max_tri_in > MS_MAX_TRIANGLES) return REGNET_ERR_UNSUPPORTED;
  return REGNET_OK;
}

}  // namespace

extern "C" int64_t regnet_mesh_simplify_workspace_bytes(int64_t G, int64_t max_tri_in) {
  return ms_sizes(G, max_tri_in) == REGNET_OK ? ms_layout(G, max_tri_in).total : -1;
}

extern "C" int64_t regnet_mesh_simplify_table_slots(int64_t max_tri_in) {
  return ms_sizes(1, max_tri_in) == REGNET_OK ? ms_slots(max_tri_in) : -1;
}

extern "C" int64_t regnet_mesh_simplify_home_slot_host(uint64_t key, int64_t slots) {
  if (slots < 2 || slots > 2 * MS_MAX_TRIANGLES || (slots & (slots - 1)) != 0) return -1;
  return (int64_t)ms_home(key, ms_log2(slots));
}

extern "C" int regnet_mesh_simplify_f32(const float* xyz, const float* normal, const float* rgb, int64_t rows,
                                        const int32_t* K_source, const int32_t* tri, int64_t max_tri_in,
                                        const int32_t* num_tri_in, const float* origin3, double cell, int64_t gx, int64_t gy,
                                        int64_t gz, int dedupe, int64_t max_vertices, int64_t max_triangles, void* workspace,
                                        float* out_xyz, float* out_normal, float* out_rgb, int32_t* out_weight, int32_t* out_tri,
                                        int32_t* num, int32_t* surface_num, void* stream) {
  if (rows < 1 || max_tri_in < 1 || gx < 1 || gy < 1 || gz < 1 || max_vertices < 1 || max_triangles < 1 ||
      (dedupe != 0 && dedupe != 1))
    return REGNET_ERR_SHAPE;
  const float cell_f = (float)cell;
  if (gx > MS_MAX_CELLS || gy > MS_MAX_CELLS || gz > MS_MAX_CELLS || gx * gy > MS_MAX_CELLS || gx * gy * gz > MS_MAX_CELLS ||
      rows > MS_MAX_VERTICES || max_vertices > MS_MAX_VERTICES || max_triangles > MS_MAX_TRIANGLES ||
      max_tri_in > MS_MAX_TRIANGLES || !(cell > 0.0 && cell < __builtin_inf()) ||
      !(cell_f > 0.0f && cell_f < __builtin_inff()))
    return REGNET_ERR_UNSUPPORTED;
  if (!xyz || !normal || !rgb || !K_source || !tri || !num_tri_in || !origin3 || !workspace || !out_xyz || !out_normal ||
      !out_rgb || !out_weight || !out_tri || !num)
    return REGNET_ERR_NULL;
  if (((uintptr_t)workspace & 7u) != 0) return REGNET_ERR_UNSUPPORTED;      // 64-bit atomics on its words
  const int64_t G = gx * gy * gz, S = ms_slots(max_tri_in);
  const MsLayout L = ms_layout(G, max_tri_in);
  MsGrid grid;
  for (int k = 0; k < 3; ++k) grid.o[k] = origin3[k];
  grid.cell = cell_f;
  grid.g[0] = (int)gx; grid.g[1] = (int)gy; grid.g[2] = (int)gz; grid.G = (int)G;
  char* ws = (char*)workspace;
  int* hdr = (int*)(ws + L.hdr);
  unsigned long long* sums = (unsigned long long*)(ws + L.sums);
  int *count = (int*)(ws + L.count), *ncount = (int*)(ws + L.ncount), *mark = (int*)(ws + L.mark);
  unsigned long long* keys = (unsigned long long*)(ws + L.keys);
  unsigned *min_row = (unsigned*)(ws + L.min_row), *first = (unsigned*)(ws + L.first);
  unsigned long long* tri_key = (unsigned long long*)(ws + L.tri_key);
  int *tri_slot = (int*)(ws + L.tri_slot), *cell_blocks = (int*)(ws + L.cell_blocks), *tri_blocks = (int*)(ws + L.tri_blocks);
  hipStream_t st = as_stream(stream);
  hipError_t e = hipMemsetAsync(ws, 0, (size_t)L.zero_end, st);
  if (e == hipSuccess)                                // without dedupe the set is not used: only the cells' first rows
    e = dedupe ? hipMemsetAsync(ws + L.keys, 0xff, (size_t)(L.ones_end - L.keys), st)
               : hipMemsetAsync(ws + L.first, 0xff, (size_t)(4 * G), st);
  if (e != hipSuccess) return (int)e;
  const unsigned row_wgs = (unsigned)ms_blocks(rows), tri_wgs = (unsigned)ms_blocks(max_tri_in), cell_wgs = (unsigned)ms_blocks(G);
  hipLaunchKernelGGL(ms_vertex_kernel, dim3(row_wgs), dim3(MS_BLOCK), 0, st, xyz, normal, rgb, K_source, (int)rows, grid, hdr,
                     sums, count, ncount, first);
  REGNET_LAUNCH_CHECK();
  hipLaunchKernelGGL(ms_insert_kernel, dim3(tri_wgs), dim3(MS_BLOCK), 0, st, xyz, K_source, (int)rows, tri, num_tri_in,
                     (int)max_tri_in, grid, dedupe, (unsigned)(S - 1), ms_log2(S), hdr, keys, min_row, tri_key, tri_slot);
  REGNET_LAUNCH_CHECK();
  hipLaunchKernelGGL(ms_survive_kernel, dim3(tri_wgs), dim3(MS_BLOCK), 0, st, num_tri_in, (int)max_tri_in, dedupe, (int)G,
                     (const unsigned*)min_row, tri_key, (const int*)tri_slot, mark, hdr, tri_blocks);
  REGNET_LAUNCH_CHECK();
  hipLaunchKernelGGL(ms_cell_count_kernel, dim3(cell_wgs), dim3(MS_BLOCK), 0, st, (const int*)mark, (const int*)count, (int)G,
                     hdr, cell_blocks);
  REGNET_LAUNCH_CHECK();
  hipLaunchKernelGGL(ms_scan_kernel, dim3(1), dim3(MS_SCAN), 0, st, cell_blocks, (int)cell_wgs, tri_blocks, (int)tri_wgs, hdr);
  REGNET_LAUNCH_CHECK();
  hipLaunchKernelGGL(ms_vertex_emit_kernel, dim3(cell_wgs), dim3(MS_BLOCK), 0, st, xyz, normal, rgb, grid,
                     (const unsigned long long*)sums, (const int*)count, (const int*)ncount, (const unsigned*)first, mark,
                     (const int*)cell_blocks, (int)max_vertices, out_xyz, out_normal, out_rgb, out_weight);
  REGNET_LAUNCH_CHECK();
  hipLaunchKernelGGL(ms_tri_emit_kernel, dim3(tri_wgs), dim3(MS_BLOCK), 0, st, num_tri_in, (int)max_tri_in, (int)G,
                     (const unsigned long long*)tri_key, (const int*)mark, (const int*)tri_blocks, (int)max_vertices,
                     (int)max_triangles, out_tri, hdr);
  REGNET_LAUNCH_CHECK();
  const int64_t tail = max_vertices > max_triangles ? max_vertices : max_triangles;
  hipLaunchKernelGGL(ms_tail_kernel, dim3((unsigned)ms_blocks(tail)), dim3(MS_BLOCK), 0, st, (const int*)hdr, K_source, (int)rows,
                     (int)max_vertices, (int)max_triangles, out_xyz, out_normal, out_rgb, out_weight, out_tri, num, surface_num);
  REGNET_LAUNCH_CHECK();
  return REGNET_OK;
}
