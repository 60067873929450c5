// tsdf_mesh.hip -- the triangle mesh of a TSDF volume on the device (gfx950): marching cubes over the surface tsdf.hip extracts.
//
// The contract is DESIGN.md par. 5 "Triangle mesh" and include/regnet_hip.h.  The vertices ARE the rows of regnet_tsdf_emit_f32
// (one per sign-changing voxel edge, in key order); this file adds the index buffer.  Integer work only: the two compares D < 0
// and D < 1 are the only floating-point operations, so there is nothing to round and tests/tsdf_mesh_reference.py restates it
// with plain loops.  The 256-case table is derived at compile time (tsdf_mesh_table.h) and lives in __constant__ memory.
//
//   * tsdf_mesh_count_kernel: blocks of 256 consecutive cells (a cell is addressed by the linear index of its low corner voxel,
//     so the blocks are tsdf_count_kernel's), ix on the lane: the eight corner loads of a wave are contiguous runs of D and W.
//     16 blocks per workgroup, one after the other (TS_CB's reason); leaves the triangles per block.  No atomic.
//   * (the caller's exclusive prefix sum)
//   * tsdf_mesh_rows_kernel: the edge-to-row lookup.  Recomputes the surface's predicate and ranks it as tsdf_emit_kernel does,
//     and leaves per voxel ONE word in the scratch plane: (first row << 3) | kept axes.  The row of candidate (v, a) is then the
//     first row plus the kept axes below a: one gathered word per triangle corner, whichever of the seven neighbouring voxels
//     (and whichever block) owns the edge.  A dense plane and not a per-64-voxel base with ballots: the cell pass would have to
//     recompute the predicate of up to seven voxels, 4 loads each, for every corner it looks up; the plane costs 4 bytes per
//     voxel of scratch, of which only the voxels with a kept candidate are ever written or read.
//   * tsdf_mesh_emit_kernel: recomputes the case, ranks the triangles of a block in cell order (three ballots over the bits of
//     the per-cell count, the waves' totals through LDS) and writes row tri_block_base[b] + rank.
//   * tsdf_mesh_tail_kernel: the -1 rows beyond Kt, and num_tri.
// A workgroup of the rows and emit passes whose block has no candidate / no triangle leaves at once: outside the surface's
// shell the volume is not read again.  The launches are ordered by the stream: no workgroup waits for another, no flags, no
// cooperative launch.
#include "tsdf_mesh_table.h"
#include "tsdf_volume.h"

namespace {

constexpr long long TM_MAX_VOXELS = 1ll << 28;
constexpr long long TM_MAX_TRIANGLES = 1ll << 22;
constexpr int TM_BLOCK = 256;
constexpr int TM_WAVES = TM_BLOCK / 64;
constexpr int TM_CB = 16;                           // blocks of 256 cells per workgroup of the count pass (tsdf.hip's TS_CB)
constexpr int TM_ROW_CAP = (1 << 28) - 1;           // a first row is stored in 28 bits; K <= 2^21, so a capped row is beyond it

constexpr tsdf_mesh::Table TM_HOST_TABLE = tsdf_mesh::make_table();
__constant__ tsdf_mesh::Table tm_table = tsdf_mesh::make_table();

__global__ __launch_bounds__(64) void tsdf_mesh_clear_kernel(int32_t* __restrict__ num_tri) {
  if (threadIdx.x < 4) num_tri[threadIdx.x] = 0;
}

// the case of cell l: the mask of its corners with D < 0, or 0 (no triangle) when l is no cell or a corner is not usable
__device__ __forceinline__ int mesh_case(const float* __restrict__ D, const int32_t* __restrict__ W, const ExtractArgs& a, int l) {
  if (l >= a.n) return 0;
  int ix, iy, iz;
  tsdf_index(a, l, ix, iy, iz);
  if (ix + 1 >= a.nx || iy + 1 >= a.ny || iz + 1 >= a.nz) return 0;
  const int sy = a.nx, sz = a.nx * a.ny;
  int cs = 0;
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    const int m = l + (c & 1) + (c >> 1 & 1) * sy + (c >> 2 & 1) * sz;      // inside the volume: the three tests above
    if (W[m] < a.min_weight) return 0;
    const float d = D[m];
    if (!(d < 1.0f)) return 0;
    cs |= (d < 0.0f ? 1 : 0) << c;
  }
  return cs;
}

__global__ __launch_bounds__(TM_BLOCK) void tsdf_mesh_count_kernel(const float* __restrict__ D, const int32_t* __restrict__ W,
                                                                   const ExtractArgs a, int32_t* __restrict__ tri_block_counts) {
  __shared__ int s_tri[TM_WAVES];
  const int blocks = (a.n + TM_BLOCK - 1) / TM_BLOCK;
  const int first = (int)blockIdx.x * TM_CB, last = min(first + TM_CB, blocks);
  for (int block = first; block < last; ++block) {
    const int t = tm_table.triangles[mesh_case(D, W, a, block * TM_BLOCK + (int)threadIdx.x)];
    const int wave_total = __popcll(__ballot(t & 1)) + 2 * __popcll(__ballot(t & 2)) + 4 * __popcll(__ballot(t & 4));
    block_put(wave_total, s_tri);
    __syncthreads();
    if (threadIdx.x == 0) tri_block_counts[block] = block_sum<TM_WAVES>(s_tri);
    __syncthreads();
  }
}

__global__ __launch_bounds__(TM_BLOCK) void tsdf_mesh_rows_kernel(const float* __restrict__ D, const int32_t* __restrict__ W,
                                                                  const ExtractArgs a, const int32_t* __restrict__ block_counts,
                                                                  const int32_t* __restrict__ block_base,
                                                                  int32_t* __restrict__ first_row) {
  __shared__ int s_total[TM_WAVES];
  if (block_counts[blockIdx.x] == 0) return;          // (the whole workgroup)
  const int l = (int)(blockIdx.x * (unsigned)TM_BLOCK + threadIdx.x);
  int bits = 0;
  if (l < a.n) {
    bool observed;
    int ix, iy, iz;
    tsdf_index(a, l, ix, iy, iz);
    bits = tsdf_kept(D, W, a, l, ix, iy, iz, observed);
  }
  const uint64_t b0 = __ballot(bits & 1), b1 = __ballot(bits & 2), b2 = __ballot(bits & 4);
  const int wave = threadIdx.x >> 6;
  if (lane_id() == 0) s_total[wave] = __popcll(b0) + __popcll(b1) + __popcll(b2);
  __syncthreads();
  if (bits == 0) return;
  long long row = (long long)block_base[blockIdx.x] + mbcnt64(b0) + mbcnt64(b1) + mbcnt64(b2);      // tsdf_emit_kernel's
  for (int w = 0; w < wave; ++w) row += s_total[w];
  first_row[l] = (int32_t)((row < TM_ROW_CAP ? row : TM_ROW_CAP) << 3) | bits;
}

__global__ __launch_bounds__(TM_BLOCK) void tsdf_mesh_emit_kernel(const float* __restrict__ D, const int32_t* __restrict__ W,
                                                                  const ExtractArgs a, const int32_t* __restrict__ first_row,
                                                                  const int32_t* __restrict__ K_source,
                                                                  const int32_t* __restrict__ tri_block_counts,
                                                                  const int32_t* __restrict__ tri_block_base, int max_triangles,
                                                                  int32_t* __restrict__ tri, int32_t* __restrict__ num_tri) {
  __shared__ int s_total[TM_WAVES], s_dropped[TM_WAVES];
  if (tri_block_counts[blockIdx.x] == 0) return;      // (the whole workgroup)
  const int l = (int)(blockIdx.x * (unsigned)TM_BLOCK + threadIdx.x);
  const int cs = mesh_case(D, W, a, l);
  const int t = tm_table.triangles[cs];
  const uint64_t m0 = __ballot(t & 1), m1 = __ballot(t & 2), m2 = __ballot(t & 4);
  const int wave = threadIdx.x >> 6;
  if (lane_id() == 0) s_total[wave] = __popcll(m0) + 2 * __popcll(m1) + 4 * __popcll(m2);
  __syncthreads();
  long long row = (long long)tri_block_base[blockIdx.x] + mbcnt64(m0) + 2 * mbcnt64(m1) + 4 * mbcnt64(m2);
  for (int w = 0; w < wave; ++w) row += s_total[w];
  const int K = K_source[0];
  const int sy = a.nx, sz = a.nx * a.ny;
  int dropped = 0;
  for (int j = 0; j < t && row < max_triangles; ++j, ++row) {      // (rows ascend: every later one is beyond the end too)
    int r[3];
    bool whole = true;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const int e = tm_table.edges[cs][3 * j + k];
      const int c = tm_table.edge_corner[e], axis = tm_table.edge_axis[e];
      const int word = first_row[l + (c & 1) + (c >> 1 & 1) * sy + (c >> 2 & 1) * sz];
      r[k] = (word >> 3) + __popc((unsigned)word & ((1u << axis) - 1u));
      whole = whole && r[k] < K;
    }
    if (!whole) ++dropped;
#pragma unroll
    for (int k = 0; k < 3; ++k) tri[row * 3 + k] = whole ? r[k] : -1;
  }
  block_put(wave_sum(dropped), s_dropped);
  __syncthreads();
  if (threadIdx.x == 0) {
    const int d = block_sum<TM_WAVES>(s_dropped);
    if (d != 0) atomicAdd(&num_tri[2], d);            // one integer atomic per workgroup
  }
}

__global__ __launch_bounds__(TM_BLOCK) void tsdf_mesh_tail_kernel(const int32_t* __restrict__ tri_block_counts,
                                                                  const int32_t* __restrict__ tri_block_base, int blocks,
                                                                  int max_triangles, int32_t* __restrict__ tri,
                                                                  int32_t* __restrict__ num_tri) {
  const long long total = (long long)tri_block_base[blocks - 1] + tri_block_counts[blocks - 1];
  const int Kt = (int)(total < max_triangles ? total : max_triangles);
  const long long row = (long long)blockIdx.x * TM_BLOCK + threadIdx.x;
  if (row == 0) {
    num_tri[0] = Kt;
    num_tri[1] = (int32_t)total;
    num_tri[3] = total > max_triangles ? 1 : 0;
  }
  if (row < Kt || row >= max_triangles) return;
#pragma unroll
  for (int k = 0; k < 3; ++k) tri[row * 3 + k] = -1;
}

int mesh_dims(int64_t nx, int64_t ny, int64_t nz) {
  if (nx < 1 || ny < 1 || nz < 1) return REGNET_ERR_SHAPE;
  if (nx > TM_MAX_VOXELS || ny > TM_MAX_VOXELS || nz > TM_MAX_VOXELS || nx * ny > TM_MAX_VOXELS || nx * ny * nz > TM_MAX_VOXELS)
    return REGNET_ERR_UNSUPPORTED;
  return REGNET_OK;
}

ExtractArgs mesh_args(int64_t nx, int64_t ny, int64_t nz, int64_t min_weight) {
  ExtractArgs a;
  a.nx = (int)nx; a.ny = (int)ny; a.nz = (int)nz; a.n = (int)(nx * ny * nz);
  a.min_weight = (int)(min_weight < 0x7FFFFFFF ? min_weight : 0x7FFFFFFF);
  return a;
}

}  // namespace

extern "C" int64_t regnet_tsdf_mesh_blocks(int64_t nx, int64_t ny, int64_t nz) {
  return mesh_dims(nx, ny, nz) == REGNET_OK ? (nx * ny * nz + TM_BLOCK - 1) / TM_BLOCK : -1;
}

extern "C" int64_t regnet_tsdf_mesh_scratch_bytes(int64_t nx, int64_t ny, int64_t nz) {
  return mesh_dims(nx, ny, nz) == REGNET_OK ? 4 * nx * ny * nz : -1;
}

extern "C" int regnet_tsdf_mesh_case(int64_t case_index, int8_t* edges16) {
  if (case_index < 0 || case_index >= tsdf_mesh::CASES) return REGNET_ERR_SHAPE;
  if (!edges16) return REGNET_ERR_NULL;
  for (int i = 0; i < tsdf_mesh::SLOTS; ++i) edges16[i] = TM_HOST_TABLE.edges[case_index][i];
  return REGNET_OK;
}

extern "C" int regnet_tsdf_mesh_count(const void* volume, int64_t nx, int64_t ny, int64_t nz, int64_t min_weight,
                                      int32_t* tri_block_counts, int32_t* num_tri, void* stream) {
  const int bad = mesh_dims(nx, ny, nz);
  if (bad == REGNET_ERR_SHAPE || min_weight < 1) return REGNET_ERR_SHAPE;
  if (bad != REGNET_OK) return bad;
  if (!volume || !tri_block_counts || !num_tri) return REGNET_ERR_NULL;
  const ExtractArgs a = mesh_args(nx, ny, nz, min_weight);
  const Planes p = planes_of(const_cast<void*>(volume), a.n);
  hipStream_t s = as_stream(stream);
  hipLaunchKernelGGL(tsdf_mesh_clear_kernel, dim3(1), dim3(64), 0, s, num_tri);
  REGNET_LAUNCH_CHECK();
  const int blocks = (a.n + TM_BLOCK - 1) / TM_BLOCK;
  hipLaunchKernelGGL(tsdf_mesh_count_kernel, dim3((unsigned)((blocks + TM_CB - 1) / TM_CB)), dim3(TM_BLOCK), 0, s, p.D, p.W, a,
                     tri_block_counts);
  REGNET_LAUNCH_CHECK();
  return REGNET_OK;
}

extern "C" int regnet_tsdf_mesh_emit(const void* volume, int64_t nx, int64_t ny, int64_t nz, int64_t min_weight,
                                     const int32_t* block_counts, const int32_t* block_base, const int32_t* K_source,
                                     const int32_t* tri_block_counts, const int32_t* tri_block_base, int64_t max_triangles,
                                     void* scratch, int32_t* tri, int32_t* num_tri, void* stream) {
  const int bad = mesh_dims(nx, ny, nz);
  if (bad == REGNET_ERR_SHAPE || min_weight < 1 || max_triangles < 1) return REGNET_ERR_SHAPE;
  if (bad != REGNET_OK) return bad;
  if (max_triangles > TM_MAX_TRIANGLES) return REGNET_ERR_UNSUPPORTED;
  if (!volume || !block_counts || !block_base || !K_source || !tri_block_counts || !tri_block_base || !scratch || !tri || !num_tri)
    return REGNET_ERR_NULL;
  const ExtractArgs a = mesh_args(nx, ny, nz, min_weight);
  const Planes p = planes_of(const_cast<void*>(volume), a.n);
  const int blocks = (a.n + TM_BLOCK - 1) / TM_BLOCK;
  int32_t* first_row = (int32_t*)scratch;
  hipStream_t s = as_stream(stream);
  hipLaunchKernelGGL(tsdf_mesh_rows_kernel, dim3((unsigned)blocks), dim3(TM_BLOCK), 0, s, p.D, p.W, a, block_counts, block_base,
                     first_row);
  REGNET_LAUNCH_CHECK();
  hipLaunchKernelGGL(tsdf_mesh_emit_kernel, dim3((unsigned)blocks), dim3(TM_BLOCK), 0, s, p.D, p.W, a, first_row, K_source,
                     tri_block_counts, tri_block_base, (int)max_triangles, tri, num_tri);
  REGNET_LAUNCH_CHECK();
  hipLaunchKernelGGL(tsdf_mesh_tail_kernel, dim3((unsigned)((max_triangles + TM_BLOCK - 1) / TM_BLOCK)), dim3(TM_BLOCK), 0, s,
                     tri_block_counts, tri_block_base, blocks, (int)max_triangles, tri, num_tri);
  REGNET_LAUNCH_CHECK();
  return REGNET_OK;
}
