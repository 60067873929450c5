// cluster.hip -- Euclidean cluster extraction over one cloud on the device (gfx950): the connected components of the graph
// "d2 <= T2" over the graph rows (mask set, coordinates finite), the largest of them as objects with size, first row and
// bounding box, and the assignment of query points (grasp centres) to objects.  Built with -ffp-contract=off: d2 is sqdist3,
// three individually rounded products summed left to right, so tests/cluster_reference.py decides every edge the same way; the
// grid (grid.h) only decides WHICH pairs are evaluated.  Contract: include/regnet_hip.h, DESIGN.md par. 5.
//
//   stage 1  cl_init_kernel     parent[i] = i for graph rows, -1 otherwise; the graph rows compacted (wave-aggregated atomicAdd,
//                               any order) so that excluded rows never reach the grid
//            build_grid         over the compacted rows, cell edge >= tolerance, the row count read on the device
//            cl_union_kernel    a thread per graph row scans the cells overlapping its ball and unites with every in-tolerance
//                               row of higher index: lock-free union-find, the larger root hooked under the smaller by atomicCAS
//            cl_flatten_kernel  root[i] = the root of i = the smallest row of its component; component sizes by integer atomics
//            cl_key_kernel      key[r] = size of the component rooted at r when it is kept (>= min_points), else 0; kept count
//   (the caller ranks: a stable descending sort of `key`, whose index is the root, is "size descending, equal sizes by root")
//   stage 2  cl_tables_kernel   the first max_objects ranks become the object tables; root -> object id
//            cl_label_kernel    label[i]; the boxes by atomicMin / atomicMax on order-preserving integer keys of the coordinates
//            cl_bbox_kernel     keys back to floats
// Parent pointers only ever decrease (parent[x] <= x), every loop below walks strictly downwards, and no thread waits for
// another: a failed atomicCAS continues from the value it returned.  Parent reads are agent-scope atomic loads, so a stale
// line in a CU's vector cache is never taken for the current pointer.
#include "grid.h"

namespace {

constexpr int CL_LDS_OBJECTS = 256;   // objects whose box is reduced in LDS before the global atomics

struct ClusterLayout {   // byte offsets into the workspace
  long long cnt, src, cxyz, parent, objid, grid, total;
};

__host__ inline ClusterLayout cluster_layout(long long N) {
  auto up = [](long long b) { return (b + 15) / 16 * 16; };
  ClusterLayout L;
  L.cnt = 0;                         // int32[4]: graph rows, kept components
  L.src = 16;                        // int32[N]: compacted row -> source row
  L.cxyz = L.src + up(N * 4);        // float[3 N]: compacted coordinates
  L.parent = L.cxyz + up(N * 12);    // int32[N], by source row
  L.objid = L.parent + up(N * 4);    // int32[N]: root -> object id, -1
  L.grid = L.objid + up(N * 4);
  L.total = L.grid + up(grid_slab_bytes(N));
  return L;
}

__device__ __forceinline__ bool finite3(float x, float y, float z) {
  return fabsf(x) < __builtin_inff() && fabsf(y) < __builtin_inff() && fabsf(z) < __builtin_inff();   // (NaN fails)
}

__global__ __launch_bounds__(256) void cl_init_kernel(const float* __restrict__ xyz, const uint8_t* __restrict__ mask, int N,
                                                      int* __restrict__ cnt, int* __restrict__ src, float* __restrict__ cxyz,
                                                      int* __restrict__ parent, int* __restrict__ objid,
                                                      int* __restrict__ key) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  float x = 0.f, y = 0.f, z = 0.f;
  bool valid = false;
  if (i < N) {
    x = xyz[(int64_t)i * 3]; y = xyz[(int64_t)i * 3 + 1]; z = xyz[(int64_t)i * 3 + 2];
    valid = (mask == nullptr || mask[i] != 0) && finite3(x, y, z);
    parent[i] = valid ? i : -1;
    objid[i] = -1;
    key[i] = 0;
  }
  const int c = wave_append(valid, &cnt[0]);
  if (valid) {
    src[c] = i;
    cxyz[(int64_t)c * 3] = x; cxyz[(int64_t)c * 3 + 1] = y; cxyz[(int64_t)c * 3 + 2] = z;
  }
}

__device__ __forceinline__ int cl_load(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// the root of x, halving the path on the way (atomicMin: a pointer is only ever lowered, to another ancestor)
__device__ __forceinline__ int cl_find(int* __restrict__ parent, int x) {
  int p = cl_load(&parent[x]);
  while (p != x) {
    const int g = cl_load(&parent[p]);
    if (g != p) atomicMin(&parent[x], g);
    x = p;
    p = g;
  }
  return x;
}

__device__ __forceinline__ void cl_unite(int* __restrict__ parent, int a, int b) {
  for (;;) {
    a = cl_find(parent, a);
    b = cl_find(parent, b);
    if (a == b) return;
    const int hi = max(a, b), lo = min(a, b);
    const int old = atomicCAS(&parent[hi], hi, lo);
    if (old == hi) return;
    a = old;   // hi was hooked meanwhile, under old < hi: go on from there
    b = lo;
  }
}

__global__ __launch_bounds__(256) void cl_union_kernel(const float* __restrict__ cxyz, const int* __restrict__ src,
                                                       const int* __restrict__ cnt, int N, float T2, float tolerance,
                                                       const char* __restrict__ slab, int* __restrict__ parent) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= min(N, cnt[0])) return;
  const GridHeader H = *reinterpret_cast<const GridHeader*>(slab);
  const int* cell_start = grid_cell_start(const_cast<char*>(slab));
  const float4* sorted = grid_sorted(const_cast<char*>(slab));
  const int i = src[c];
  const float qx = cxyz[(int64_t)c * 3], qy = cxyz[(int64_t)c * 3 + 1], qz = cxyz[(int64_t)c * 3 + 2];
  const float pad = tolerance * 1.0001f + H.eps + 4e-6f * fmaxf(fmaxf(fabsf(qx), fabsf(qy)), fabsf(qz));   // conservative cell range of the ball
  const int x0 = cell_coord(qx - pad, H.lo[0], H.inv_h, H.dim[0]), x1 = cell_coord(qx + pad, H.lo[0], H.inv_h, H.dim[0]);
  const int y0 = cell_coord(qy - pad, H.lo[1], H.inv_h, H.dim[1]), y1 = cell_coord(qy + pad, H.lo[1], H.inv_h, H.dim[1]);
  const int z0 = cell_coord(qz - pad, H.lo[2], H.inv_h, H.dim[2]), z1 = cell_coord(qz + pad, H.lo[2], H.inv_h, H.dim[2]);
  for (int z = z0; z <= z1; ++z)
    for (int y = y0; y <= y1; ++y) {
      const int row = (z * H.dim[1] + y) * H.dim[0];
      const int beg = cell_start[row + x0], end = cell_start[row + x1 + 1];   // the x-run of cells is contiguous
      for (int k = beg; k < end; ++k) {
        const float4 p = sorted[k];
        if (!(sqdist3(qx, qy, qz, p.x, p.y, p.z) <= T2)) continue;
        const int j = src[__float_as_int(p.w)];
        if (j > i) cl_unite(parent, i, j);
      }
    }
}

__global__ __launch_bounds__(256) void cl_flatten_kernel(int* __restrict__ parent, int N, int* __restrict__ root,
                                                         int* __restrict__ key) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  int r = -1;
  if (i < N) {
    if (parent[i] >= 0) r = cl_find(parent, i);
    root[i] = r;
  }
  // component sizes: the lanes of a wave that share a root add once (four rounds, then one atomic per lane)
  bool todo = r >= 0;
  for (int round = 0; round < 4; ++round) {
    const uint64_t votes = __ballot(todo);
    if (votes == 0ull) break;
    const int leader = __builtin_ctzll(votes);
    const int r0 = __shfl(r, leader, 64);
    const bool same = todo && r == r0;
    const uint64_t group = __ballot(same);
    if (lane_id() == leader) atomicAdd(&key[r0], (int)__popcll(group));
    todo = todo && !same;
  }
  if (todo) atomicAdd(&key[r], 1);
}

__global__ __launch_bounds__(256) void cl_key_kernel(const int* __restrict__ root, int N, int min_points, int* __restrict__ key,
                                                     int* __restrict__ cnt) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  bool kept = false;
  if (i < N && root[i] == i) {
    kept = key[i] >= min_points;
    if (!kept) key[i] = 0;
  }
  wave_append(kept, &cnt[1]);   // (only the count is wanted)
}

// order-preserving integer key of a float (-0.0 below +0.0) and back
__device__ __forceinline__ unsigned cl_float_key(float v) {
  const unsigned u = __float_as_uint(v);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float cl_key_float(unsigned k) {
  return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}

__global__ __launch_bounds__(256) void cl_tables_kernel(const long long* __restrict__ order, const int* __restrict__ key,
                                                        const int* __restrict__ cnt, int N, int K, int ranked,
                                                        int* __restrict__ objid, int* __restrict__ num,
                                                        int* __restrict__ object_size, int* __restrict__ object_first,
                                                        unsigned* __restrict__ bbox) {
  const int r = blockIdx.x * 256 + threadIdx.x;
  if (r >= K) return;
  auto object_at = [&](int q) -> long long {   // the root of rank q, or -1 when rank q is no kept component
    if (q >= ranked) return -1;
    const long long o = order[q];
    return (o >= 0 && o < N && key[o] > 0) ? o : -1;
  };
  const long long o = object_at(r);
  object_size[r] = o >= 0 ? key[o] : -1;
  object_first[r] = (int)o;
  if (o >= 0) objid[o] = r;
#pragma unroll
  for (int a = 0; a < 6; ++a) bbox[r * 6ll + a] = o >= 0 ? (a < 3 ? 0xffffffffu : 0u) : 0x7fc00000u;
  // the kept components are a prefix of the ranks (key > 0 sorts before key == 0): its end is the object count
  if (o >= 0 && (r + 1 == K || object_at(r + 1) < 0)) num[0] = r + 1;
  if (r == 0) {
    if (o < 0) num[0] = 0;
    num[1] = cnt[1];
  }
}

__global__ __launch_bounds__(256) void cl_label_kernel(const float* __restrict__ xyz, const int* __restrict__ root,
                                                       const int* __restrict__ objid, int N, int* __restrict__ label,
                                                       unsigned* __restrict__ bbox) {
  __shared__ unsigned s_box[CL_LDS_OBJECTS][6];
  for (int t = threadIdx.x; t < CL_LDS_OBJECTS * 6; t += 256) s_box[t / 6][t % 6] = (t % 6) < 3 ? 0xffffffffu : 0u;
  __syncthreads();
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < N) {
    const int r = root[i];
    const int l = r >= 0 ? objid[r] : -1;
    label[i] = l;
    if (l >= 0) {
      unsigned* box = l < CL_LDS_OBJECTS ? s_box[l] : bbox + l * 6ll;
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        const unsigned k = cl_float_key(xyz[(int64_t)i * 3 + a]);
        atomicMin(&box[a], k);
        atomicMax(&box[3 + a], k);
      }
    }
  }
  __syncthreads();
  for (int t = threadIdx.x; t < CL_LDS_OBJECTS * 6; t += 256) {
    const int l = t / 6, a = t % 6;
    const unsigned k = s_box[l][a];
    if (a < 3 ? k != 0xffffffffu : k != 0u) {   // touched by this workgroup: object l exists
      if (a < 3) atomicMin(&bbox[l * 6ll + a], k); else atomicMax(&bbox[l * 6ll + a], k);
    }
  }
}

__global__ __launch_bounds__(256) void cl_bbox_kernel(const int* __restrict__ object_size, int K, unsigned* __restrict__ bbox) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= K * 6ll) return;
  if (object_size[t / 6] >= 0) bbox[t] = __float_as_uint(cl_key_float(bbox[t]));
}

// A wave per query: every lane keeps the best (d2, row) of its rows, then the wave reduces.
__global__ __launch_bounds__(256) void cl_assign_kernel(const float* __restrict__ query, int Q, const float* __restrict__ xyz,
                                                        const int* __restrict__ label, int N, float R2,
                                                        int* __restrict__ object, int* __restrict__ point) {
  const int lane = lane_id();
  const long long q = blockIdx.x * 4ll + (threadIdx.x >> 6);
  if (q >= Q) return;   // wave-uniform
  const float qx = query[q * 3], qy = query[q * 3 + 1], qz = query[q * 3 + 2];
  float bd = __builtin_inff();
  int bj = 0x7fffffff;
  if (finite3(qx, qy, qz)) {
    for (int j = lane; j < N; j += 64) {
      if (label[j] < 0) continue;
      const float d2 = sqdist3(qx, qy, qz, xyz[(int64_t)j * 3], xyz[(int64_t)j * 3 + 1], xyz[(int64_t)j * 3 + 2]);
      if (d2 <= R2 && (d2 < bd || (d2 == bd && j < bj))) { bd = d2; bj = j; }
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const float od = __shfl_xor(bd, off, 64);
    const int oj = __shfl_xor(bj, off, 64);
    if (oj != 0x7fffffff && (bj == 0x7fffffff || od < bd || (od == bd && oj < bj))) { bd = od; bj = oj; }
  }
  if (lane == 0) {
    const bool found = bj != 0x7fffffff;
    point[q] = found ? bj : -1;
    object[q] = found ? label[bj] : -1;
  }
}

}  // namespace

extern "C" int64_t regnet_cluster_workspace_bytes(int64_t N, int64_t max_objects) {
  if (N < 0 || max_objects < 1 || N >= (int64_t)1 << 31 || max_objects > (1 << 28)) return -1;   // the limits of the launch
  return cluster_layout(N).total;
}

extern "C" int regnet_cluster_points_f32(const float* xyz, const uint8_t* mask, int64_t N, float tolerance, int64_t min_points,
                                         int64_t max_objects, int32_t* root, int32_t* key, const int64_t* order, int32_t* label,
                                         int32_t* num, int32_t* object_size, int32_t* object_first, float* object_bbox,
                                         void* workspace, int stages, void* stream) {
  if (N < 0 || min_points < 1 || max_objects < 1 || stages < 1 || stages > 3) return REGNET_ERR_SHAPE;
  if (!(tolerance > 0.f) || !(tolerance < __builtin_inff()) || N >= (int64_t)1 << 31 || max_objects > (1 << 28))
    return REGNET_ERR_UNSUPPORTED;
  const bool first = stages & 1, second = stages & 2;
  if (!workspace || (N > 0 && (!xyz || !root || !key))) return REGNET_ERR_NULL;
  if (second && (!num || !object_size || !object_first || !object_bbox || (N > 0 && (!order || !label)))) return REGNET_ERR_NULL;
  hipStream_t st = as_stream(stream);
  const ClusterLayout L = cluster_layout(N);
  char* ws = (char*)workspace;
  int* cnt = (int*)(ws + L.cnt);
  int* src = (int*)(ws + L.src);
  float* cxyz = (float*)(ws + L.cxyz);
  int* parent = (int*)(ws + L.parent);
  int* objid = (int*)(ws + L.objid);
  const dim3 per_row((unsigned)((N + 255) / 256)), wg(256);
  const int mp = (int)(min_points > N ? N + 1 : min_points);
  if (first) {
    hipError_t e = hipMemsetAsync(cnt, 0, 16, st);
    if (e != hipSuccess) return (int)e;
    if (N > 0) {
      hipLaunchKernelGGL(cl_init_kernel, per_row, wg, 0, st, xyz, mask, (int)N, cnt, src, cxyz, parent, objid, (int*)key);
      REGNET_LAUNCH_CHECK();
      int rc = build_grid(cxyz, 0, 1, 3, 1, N, tolerance, ws + L.grid, st, cnt);
      if (rc) return rc;
      const float T2 = tolerance * tolerance;
      hipLaunchKernelGGL(cl_union_kernel, per_row, wg, 0, st, cxyz, src, cnt, (int)N, T2, tolerance, ws + L.grid, parent);
      hipLaunchKernelGGL(cl_flatten_kernel, per_row, wg, 0, st, parent, (int)N, (int*)root, (int*)key);
      hipLaunchKernelGGL(cl_key_kernel, per_row, wg, 0, st, (const int*)root, (int)N, mp, (int*)key, cnt);
      REGNET_LAUNCH_CHECK();
    }
  }
  if (second) {
    const int K = (int)max_objects, ranked = (int)(N < max_objects ? N : max_objects);
    unsigned* box = (unsigned*)object_bbox;
    hipLaunchKernelGGL(cl_tables_kernel, dim3((unsigned)((K + 255) / 256)), wg, 0, st, (const long long*)order, (const int*)key,
                       (const int*)cnt, (int)N, K, ranked, objid, (int*)num, (int*)object_size, (int*)object_first, box);
    if (N > 0)
      hipLaunchKernelGGL(cl_label_kernel, per_row, wg, 0, st, xyz, (const int*)root, (const int*)objid, (int)N, (int*)label, box);
    hipLaunchKernelGGL(cl_bbox_kernel, dim3((unsigned)((K * 6ll + 255) / 256)), wg, 0, st, (const int*)object_size, K, box);
    REGNET_LAUNCH_CHECK();
  }
  return REGNET_OK;
}

extern "C" int regnet_cluster_assign_f32(const float* query, int64_t Q, const float* xyz, const int32_t* label, int64_t N,
                                         float radius, int32_t* object, int32_t* point, void* stream) {
  if (Q < 0 || N < 0) return REGNET_ERR_SHAPE;
  if (!(radius >= 0.f) || N >= (int64_t)1 << 31 || Q >= (int64_t)1 << 31) return REGNET_ERR_UNSUPPORTED;
  if (Q == 0) return REGNET_OK;
  if (!query || !object || !point || (N > 0 && (!xyz || !label))) return REGNET_ERR_NULL;
  const float R2 = radius * radius;
  hipLaunchKernelGGL(cl_assign_kernel, dim3((unsigned)((Q + 3) / 4)), dim3(256), 0, as_stream(stream), query, (int)Q, xyz,
                     (const int*)label, (int)N, R2, (int*)object, (int*)point);
  REGNET_LAUNCH_CHECK();
  return REGNET_OK;
}
