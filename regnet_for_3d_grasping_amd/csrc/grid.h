// grid.h -- the uniform grid shared by grid.hip and cluster.hip: header layout, cell helpers, the four build kernels and
// build_grid.  Everything here has internal linkage; each translation unit that includes it carries its own copy.
#pragma once
#include "common.h"

namespace {

#define GRID_MAX_CELLS 65536
#define GRID_HDR_FLOATS 16

struct GridHeader {   // per scene, at the start of its workspace slab (GRID_HDR_FLOATS * 4 bytes)
  float lo[3];
  float h;
  float inv_h;
  int dim[3];
  int cells;
  float eps;   // bound on the fp32 rounding of a cell-edge coordinate in this grid
  int pad[6];
};

static_assert(sizeof(GridHeader) == GRID_HDR_FLOATS * 4, "header layout");

__host__ __device__ inline long long grid_slab_bytes(long long N) {
  // header | cell_start[GRID_MAX_CELLS + 1] | sorted float4[N]
  long long b = GRID_HDR_FLOATS * 4 + (GRID_MAX_CELLS + 1) * 4ll;
  b = (b + 15) / 16 * 16;
  return b + N * 16ll;
}
__device__ __forceinline__ int* grid_cell_start(char* slab) { return reinterpret_cast<int*>(slab + GRID_HDR_FLOATS * 4); }
__device__ __forceinline__ float4* grid_sorted(char* slab) {
  long long off = GRID_HDR_FLOATS * 4 + (GRID_MAX_CELLS + 1) * 4ll;
  off = (off + 15) / 16 * 16;
  return reinterpret_cast<float4*>(slab + off);
}

__device__ __forceinline__ int cell_coord(float v, float lo, float inv_h, int dim) {
  int c = (int)floorf((v - lo) * inv_h);
  return c < 0 ? 0 : (c >= dim ? dim - 1 : c);
}

// ---- build ------------------------------------------------------------------------------------
// Four short launches per build: bounds + header + zeroed counters (one workgroup per scene),
// histogram (all CUs), exclusive scan of the counters (one workgroup per scene), scatter (all CUs).
// cell_start[c + 1] is cell c's counter: the histogram counts into it, the scan turns it into the
// cell's first slot, and the scatter's atomicAdd hands out the slots -- leaving it at the cell's end =
// the start of cell c + 1, so after the scatter the array is the usual CSR offset table and no
// second cursor array is needed.  (The order of points inside a cell depends on the atomics; neither
// search depends on it.)
__device__ __forceinline__ int cell_of(const GridHeader& H, float x, float y, float z) {
  return (cell_coord(z, H.lo[2], H.inv_h, H.dim[2]) * H.dim[1] + cell_coord(y, H.lo[1], H.inv_h, H.dim[1])) * H.dim[0] +
         cell_coord(x, H.lo[0], H.inv_h, H.dim[0]);
}

// GRID_WG threads per scene for the two one-workgroup-per-scene kernels (bounds, scan): 512, not 1024 -- eight waves of <= 32
// registers find room on a CU whose SIMDs hold two ~200-register chain waves each; sixteen did not (the geometry of the batches
// ahead then waited for whole CUs).  Results do not depend on it (min / max, integer sums).
#define GRID_WG 512
__global__ __launch_bounds__(GRID_WG) void grid_bounds_kernel(const float* __restrict__ xyz, int64_t sb, int64_t sc,
                                                           int64_t sn, int N, const int* __restrict__ n_dev, float h_req,
                                                           char* __restrict__ ws, long long slab) {
  __shared__ float red[6][GRID_WG / 64];
  __shared__ GridHeader hdr;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const float* base = xyz + (int64_t)blockIdx.x * sb;
  char* my = ws + (long long)blockIdx.x * slab;
  int* cell_start = grid_cell_start(my);
  if (n_dev) N = min(N, *n_dev);

  float lo[3] = {__builtin_inff(), __builtin_inff(), __builtin_inff()};
  float hi[3] = {-__builtin_inff(), -__builtin_inff(), -__builtin_inff()};
  for (int j = tid; j < N; j += GRID_WG) {
    const float x = base[(int64_t)j * sn], y = base[sc + (int64_t)j * sn], z = base[2 * sc + (int64_t)j * sn];
    lo[0] = fminf(lo[0], x); hi[0] = fmaxf(hi[0], x);
    lo[1] = fminf(lo[1], y); hi[1] = fmaxf(hi[1], y);
    lo[2] = fminf(lo[2], z); hi[2] = fmaxf(hi[2], z);
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
  __syncthreads();
  if (tid == 0) {
    float e[3], scale = 0.f;
    for (int a = 0; a < 3; ++a) {
      float l = red[a][0], hgh = red[3 + a][0];
      for (int w = 1; w < GRID_WG / 64; ++w) { l = fminf(l, red[a][w]); hgh = fmaxf(hgh, red[3 + a][w]); }
      hdr.lo[a] = l;
      e[a] = fmaxf(hgh - l, 0.f);
      scale = fmaxf(scale, fmaxf(fabsf(l), fabsf(hgh)));
    }
    hdr.eps = 4e-6f * scale + 1e-30f;
    float h = h_req;
    if (!(h > 0.f)) {  // automatic: about one point per cell, never more than ~4N cells for flat / thin clouds
      const float n = (float)(N > 0 ? N : 1);
      const float vol = fmaxf(e[0], 1e-6f) * fmaxf(e[1], 1e-6f) * fmaxf(e[2], 1e-6f);
      const float area = fmaxf(fmaxf(e[0] * e[1], e[1] * e[2]), e[0] * e[2]);
      const float len = fmaxf(fmaxf(e[0], e[1]), e[2]);
      h = fmaxf(fmaxf(cbrtf(vol / n), sqrtf(area / (4.f * n))), len / (4.f * n));
      h = fmaxf(h, 1e-6f);
    }
    for (;;) {
      long long cells = 1;
      for (int a = 0; a < 3; ++a) {
        int d = (int)floorf(e[a] / h) + 1;
        d = d < 1 ? 1 : (d > 4096 ? 4096 : d);
        hdr.dim[a] = d;
        cells *= d;
      }
      if (cells <= GRID_MAX_CELLS) { hdr.cells = (int)cells; break; }
      h *= 1.26f;
    }
    hdr.h = h;
    hdr.inv_h = 1.0f / h;
  }
  __syncthreads();
  if (tid < (int)(sizeof(GridHeader) / 4)) reinterpret_cast<int*>(my)[tid] = reinterpret_cast<const int*>(&hdr)[tid];
  const int cells = hdr.cells;
  for (int c = tid; c <= cells; c += GRID_WG) cell_start[c] = 0;
}

__global__ __launch_bounds__(256) void grid_count_kernel(const float* __restrict__ xyz, int64_t sb, int64_t sc,
                                                         int64_t sn, int N, const int* __restrict__ n_dev, char* __restrict__ ws,
                                                         long long slab) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= (n_dev ? min(N, *n_dev) : N)) return;
  char* my = ws + (long long)blockIdx.y * slab;
  const GridHeader H = *reinterpret_cast<const GridHeader*>(my);
  const float* base = xyz + (int64_t)blockIdx.y * sb;
  const int c = cell_of(H, base[(int64_t)j * sn], base[sc + (int64_t)j * sn], base[2 * sc + (int64_t)j * sn]);
  atomicAdd(&grid_cell_start(my)[c + 1], 1);
}

__global__ __launch_bounds__(GRID_WG) void grid_scan_kernel(char* __restrict__ ws, long long slab) {
  __shared__ unsigned wsum[GRID_WG / 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  char* my = ws + (long long)blockIdx.x * slab;
  const int cells = reinterpret_cast<const GridHeader*>(my)->cells;
  int* cell_start = grid_cell_start(my);
  const int per = (cells + GRID_WG - 1) / GRID_WG;
  const int beg = tid * per, end = min(cells, beg + per);
  unsigned local = 0;
  for (int c = beg; c < end; ++c) local += (unsigned)cell_start[c + 1];
  unsigned incl = local;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const unsigned o = __shfl_up(incl, off, 64);
    if (lane >= off) incl += o;
  }
  if (lane == 63) wsum[wave] = incl;
  __syncthreads();
  unsigned run = incl - local;
  for (int w = 0; w < GRID_WG / 64; ++w) run += (w < wave) ? wsum[w] : 0u;
  for (int c = beg; c < end; ++c) {   // each thread rewrites only its own chunk, after having read it
    const unsigned cnt = (unsigned)cell_start[c + 1];
    cell_start[c + 1] = (int)run;     // first slot of cell c
    run += cnt;
  }
}

__global__ __launch_bounds__(256) void grid_scatter_kernel(const float* __restrict__ xyz, int64_t sb, int64_t sc,
                                                           int64_t sn, int N, const int* __restrict__ n_dev, char* __restrict__ ws,
                                                         long long slab) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= (n_dev ? min(N, *n_dev) : N)) return;
  char* my = ws + (long long)blockIdx.y * slab;
  const GridHeader H = *reinterpret_cast<const GridHeader*>(my);
  const float* base = xyz + (int64_t)blockIdx.y * sb;
  const float x = base[(int64_t)j * sn], y = base[sc + (int64_t)j * sn], z = base[2 * sc + (int64_t)j * sn];
  const int pos = atomicAdd(&grid_cell_start(my)[cell_of(H, x, y, z) + 1], 1);
  grid_sorted(my)[pos] = make_float4(x, y, z, __int_as_float(j));
}

// n_dev: NULL, or one int32 in DEVICE memory: only the first min(N, *n_dev) points are binned (a count the host never reads);
// the workspace and the launch grids are sized by N.
static int build_grid(const float* xyz, int64_t sb, int64_t sc, int64_t sn, int64_t B, int64_t N, float h, void* ws,
                      hipStream_t st, const int* n_dev = nullptr) {
  const long long slab = grid_slab_bytes(N);
  const dim3 per_point((unsigned)((N + 255) / 256), (unsigned)B);
  hipLaunchKernelGGL(grid_bounds_kernel, dim3((unsigned)B), dim3(GRID_WG), 0, st, xyz, sb, sc, sn, (int)N, n_dev, h, (char*)ws, slab);
  if (N > 0) hipLaunchKernelGGL(grid_count_kernel, per_point, dim3(256), 0, st, xyz, sb, sc, sn, (int)N, n_dev, (char*)ws, slab);
  hipLaunchKernelGGL(grid_scan_kernel, dim3((unsigned)B), dim3(GRID_WG), 0, st, (char*)ws, slab);
  if (N > 0) hipLaunchKernelGGL(grid_scatter_kernel, per_point, dim3(256), 0, st, xyz, sb, sc, sn, (int)N, n_dev, (char*)ws, slab);
  REGNET_LAUNCH_CHECK();
  return REGNET_OK;
}

}  // namespace
