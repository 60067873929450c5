// icp.hip -- point-to-plane ICP of a source cloud onto a target cloud with normals, on the device (gfx950): the pose correction
// behind fusion.refine_poses.  Built with -ffp-contract=off: the pose, the squared distances and the match test are individually
// rounded float32 operations in the written order, so tests/icp_reference.py picks every correspondence the same way; the
// residuals, the normal equations, the solve and the pose update are float64, one rounding per operation.  No floating-point
// atomics: every sum is formed in a fixed order, so two runs agree bit for bit.  Contract: include/regnet_hip.h, DESIGN.md par. 5.
//
//   prepare   build_grid (csrc/grid.h) over the target, requested cell edge = max_dist; the grid may coarsen itself to stay within
//             GRID_MAX_CELLS.  It only decides which pairs are evaluated.
//   step, launch A  icp_correspond_kernel  a lane per visited source row: pose, the nearest target row among the cells that overlap
//             the ball of max_dist (27 cells; one more along an axis only where the rounding margin reaches into it), the
//             point-to-plane residual and the row's 28 float64 terms; a shuffle tree per wave, the waves in order, one slot of
//             partial sums per workgroup.
//   projective step, launch A  icp_project_kernel  the same lane per visited row, for a target that is the organised cloud of a
//             depth image in its camera's frame: the row's pixel in that image and the (2 window + 1)^2 pixels around it are the
//             candidates, optionally gated by the angle between the normals; no grid, no prepare.  The same tail.
//   step, launch B  icp_solve_kernel      one workgroup: the slots in ascending order, a 6x6 Cholesky, Rodrigues, the pose update,
//             the status word.
//   hand-over       icp_continue_kernel   one thread: between two levels of a coarse-to-fine registration on ONE state block, a
//             finished-but-healthy status (CONVERGED, MAX_ITER) becomes RUNNING again with a new step budget.
// Both kernels of a step return at once when the status is no longer RUNNING: a caller enqueues a fixed number of steps and
// reads the state block once.  No thread waits for another and every loop ends on its own count.
#include "grid.h"

namespace {

constexpr int ICP_BLOCK = 256;
constexpr int ICP_TERMS = 28;                    // 21 of a a^T, 6 of a r, r r
constexpr int ICP_SUMS = 29;                     // ... and the pair count
constexpr int ICP_SLOT = 32;                     // doubles per workgroup slot (256-byte rows)
constexpr int ICP_PARTS = 8;                     // launch B adds the slots in 8 contiguous runs, then the runs in order
constexpr int ICP_MAX_ITER = 64;                 // rows of the history
constexpr int64_t ICP_MAX_POINTS = (int64_t)1 << 21;

enum { ICP_RUNNING = 0, ICP_CONVERGED = 1, ICP_MAX_ITER_REACHED = 2, ICP_TOO_FEW = 3, ICP_DEGENERATE = 4 };

struct IcpState {   // the device block of one registration (regnet_icp_state_bytes)
  double pose[12];                      // rows 0..2 of the row-major 4x4 source-to-target transform
  int iteration;                        // steps run so far
  int status;
  int max_iter;                         // 1..ICP_MAX_ITER
  int pad;
  double rot_eps, trans_eps;
  double history[ICP_MAX_ITER][2];      // per step run: (pairs, rms of the residuals before the step's update)
};
static_assert(sizeof(IcpState) == 128 + 16 * ICP_MAX_ITER, "state layout");

__host__ inline int64_t icp_rows(int64_t n_source, int64_t stride) { return (n_source + stride - 1) / stride; }
__host__ inline int64_t icp_slots(int64_t rows) { return (rows + ICP_BLOCK - 1) / ICP_BLOCK; }
__host__ inline bool icp_dist_ok(double d) { return d > 0.0 && d < __builtin_inf() && (float)d > 0.f && (float)d < __builtin_inff(); }

__device__ __forceinline__ bool icp_finite(float v) { return fabsf(v) < __builtin_inff(); }   // (NaN fails)

// the tail of launch A, shared by both association modes: the accepted pair's residual and its 28 float64 terms, a shuffle tree
// per wave, the waves in order, the workgroup's slot.  Every thread of the workgroup calls it (a barrier inside).
__device__ __forceinline__ void icp_accumulate(int found, float px, float py, float pz, float qx, float qy, float qz,
                                               const float* __restrict__ normals, double (*s_part)[ICP_SLOT],
                                               double* __restrict__ partial) {
  const int tid = threadIdx.x;
  const bool paired = found >= 0;
  double t[ICP_TERMS];
#pragma unroll
  for (int c = 0; c < ICP_TERMS; ++c) t[c] = 0.0;
  if (paired) {
    const double nx = (double)normals[(int64_t)found * 3], ny = (double)normals[(int64_t)found * 3 + 1],
                 nz = (double)normals[(int64_t)found * 3 + 2];
    const double dx = (double)px, dy = (double)py, dz = (double)pz;
    const double res = ((nx * (dx - (double)qx)) + (ny * (dy - (double)qy))) + (nz * (dz - (double)qz));
    const double a[6] = {dy * nz - dz * ny, dz * nx - dx * nz, dx * ny - dy * nx, nx, ny, nz};     // (p x n, n)
    int c = 0;
#pragma unroll
    for (int u = 0; u < 6; ++u) {
#pragma unroll
      for (int v = u; v < 6; ++v) t[c++] = a[u] * a[v];
    }
#pragma unroll
    for (int u = 0; u < 6; ++u) t[21 + u] = a[u] * res;
    t[27] = res * res;
  }
#pragma unroll
  for (int c = 0; c < ICP_TERMS; ++c) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) t[c] += __shfl_xor(t[c], d, 64);       // a fixed tree: every lane ends with the wave's sum
  }
  const int pairs = (int)__popcll(__ballot(paired));
  if (lane_id() == 0) {
#pragma unroll
    for (int c = 0; c < ICP_TERMS; ++c) s_part[tid >> 6][c] = t[c];
    s_part[tid >> 6][ICP_TERMS] = (double)pairs;
  }
  __syncthreads();
  if (tid < ICP_SUMS) {
    double v = 0.0;
#pragma unroll
    for (int w = 0; w < ICP_BLOCK / 64; ++w) v += s_part[w][tid];              // the waves in order
    partial[(int64_t)blockIdx.x * ICP_SLOT + tid] = v;
  }
}

__global__ __launch_bounds__(ICP_BLOCK) void icp_correspond_kernel(const float* __restrict__ src, int stride, int rows,
                                                                   const float* __restrict__ normals, int n_target,
                                                                   const IcpState* __restrict__ state, float max_dist, float max2,
                                                                   const char* __restrict__ slab, int* __restrict__ idx_out,
                                                                   double* __restrict__ partial) {
  __shared__ double s_part[ICP_BLOCK / 64][ICP_SLOT];
  if (state->status != ICP_RUNNING) return;                    // the same word for every thread of the grid
  const int tid = threadIdx.x;
  const int k = blockIdx.x * ICP_BLOCK + tid;
  float px = 0.f, py = 0.f, pz = 0.f, qx = 0.f, qy = 0.f, qz = 0.f;
  int found = -3;                                              // -3: no row behind this lane
  if (k < rows) {
    const int64_t i = (int64_t)k * stride;
    const float x = src[i * 3], y = src[i * 3 + 1], z = src[i * 3 + 2];
    found = -2;
    if (icp_finite(x) && icp_finite(y) && icp_finite(z)) {
      found = -1;
      float r[12];
#pragma unroll
      for (int j = 0; j < 12; ++j) r[j] = (float)state->pose[j];       // rounded once, to nearest even
      px = affine3(r, x, y, z);
      py = affine3(r + 4, x, y, z);
      pz = affine3(r + 8, x, y, z);
      if (n_target > 0 && icp_finite(px) && icp_finite(py) && icp_finite(pz)) {
        const GridHeader H = *reinterpret_cast<const GridHeader*>(slab);
        const int* cell_start = grid_cell_start(const_cast<char*>(slab));
        const float4* sorted = grid_sorted(const_cast<char*>(slab));
        // conservative cell range of the ball, as grid.hip's searches: a row within max_dist is never missed at a cell edge
        const float pad = max_dist * 1.0001f + H.eps + 4e-6f * fmaxf(fmaxf(fabsf(px), fabsf(py)), fabsf(pz));
        const int x0 = cell_coord(px - pad, H.lo[0], H.inv_h, H.dim[0]), x1 = cell_coord(px + pad, H.lo[0], H.inv_h, H.dim[0]);
        const int y0 = cell_coord(py - pad, H.lo[1], H.inv_h, H.dim[1]), y1 = cell_coord(py + pad, H.lo[1], H.inv_h, H.dim[1]);
        const int z0 = cell_coord(pz - pad, H.lo[2], H.inv_h, H.dim[2]), z1 = cell_coord(pz + pad, H.lo[2], H.inv_h, H.dim[2]);
        float bd = __builtin_inff();
        int bj = 0x7fffffff;
        for (int cz = z0; cz <= z1; ++cz)
          for (int cy = y0; cy <= y1; ++cy) {
            const int row = (cz * H.dim[1] + cy) * H.dim[0];
            const int beg = cell_start[row + x0], end = cell_start[row + x1 + 1];   // the x-run of cells is contiguous
            for (int c = beg; c < end; ++c) {
              const float4 t = sorted[c];
              const float d2 = sqdist3(px, py, pz, t.x, t.y, t.z);
              const int j = __float_as_int(t.w);
              if (d2 < bd || (d2 == bd && j < bj)) { bd = d2; bj = j; qx = t.x; qy = t.y; qz = t.z; }   // (a NaN d2 never wins)
            }
          }
        if (bj != 0x7fffffff && bd <= max2) found = bj;
      }
    }
    if (idx_out != nullptr) idx_out[k] = found;
  }
  icp_accumulate(found, px, py, pz, qx, qy, qz, normals, s_part, partial);
}

struct IcpCamera {   // the target's image: intrinsics rounded once to float32, the window's half width
  int W, H, window;
  float fx, fy, cx, cy;
};

// Launch A of the projective step: the target is the organised cloud of a depth image in ITS camera's frame, so the candidates
// of a source row are the (2 window + 1)^2 pixels around the pixel it projects to -- at most 25 reads of 12 + 12 bytes a lane,
// neighbouring lanes on neighbouring pixels -- instead of the cells of a grid.  The pixel is csrc/depth.hip's depth_project()
// expression.  src_normals == nullptr: the normal gate is off.
__global__ __launch_bounds__(ICP_BLOCK) void icp_project_kernel(const float* __restrict__ src, int stride, int rows,
                                                                const float* __restrict__ src_normals,
                                                                const float* __restrict__ target,
                                                                const float* __restrict__ normals, const IcpCamera cam,
                                                                const IcpState* __restrict__ state, float max2, float min_cos,
                                                                int* __restrict__ idx_out, double* __restrict__ partial) {
  __shared__ double s_part[ICP_BLOCK / 64][ICP_SLOT];
  if (state->status != ICP_RUNNING) return;                    // the same word for every thread of the grid
  const int k = blockIdx.x * ICP_BLOCK + threadIdx.x;
  float px = 0.f, py = 0.f, pz = 0.f, qx = 0.f, qy = 0.f, qz = 0.f;
  int found = -3;                                              // -3: no row behind this lane
  if (k < rows) {
    const int64_t i = (int64_t)k * stride;
    const float x = src[i * 3], y = src[i * 3 + 1], z = src[i * 3 + 2];
    found = -2;
    if (icp_finite(x) && icp_finite(y) && icp_finite(z)) {
      found = -1;
      float r[12];
#pragma unroll
      for (int j = 0; j < 12; ++j) r[j] = (float)state->pose[j];       // rounded once, to nearest even
      px = affine3(r, x, y, z);
      py = affine3(r + 4, x, y, z);
      pz = affine3(r + 8, x, y, z);
      bool usable = icp_finite(px) && icp_finite(py) && icp_finite(pz) && pz > 0.f;
      float mx = 0.f, my = 0.f, mz = 0.f;
      if (usable && src_normals != nullptr) {
        const float sx = src_normals[i * 3], sy = src_normals[i * 3 + 1], sz = src_normals[i * 3 + 2];
        usable = icp_finite(sx) && icp_finite(sy) && icp_finite(sz);
        mx = dot3(r[0], r[1], r[2], sx, sy, sz);
        my = dot3(r[4], r[5], r[6], sx, sy, sz);
        mz = dot3(r[8], r[9], r[10], sx, sy, sz);
      }
      if (usable) {
        const float uf = (__fdiv_rn(px, pz) * cam.fx) + cam.cx;
        const float vf = (__fdiv_rn(py, pz) * cam.fy) + cam.cy;
        const float fu = floorf(uf + 0.5f), fv = floorf(vf + 0.5f);
        if (fu >= 0.0f && fu < (float)cam.W && fv >= 0.0f && fv < (float)cam.H) {      // in float: a NaN fails
          const int u = (int)fu, v = (int)fv;
          const int ulo = max(u - cam.window, 0), uhi = min(u + cam.window, cam.W - 1);
          const int vlo = max(v - cam.window, 0), vhi = min(v + cam.window, cam.H - 1);
          float bd = __builtin_inff();
          int bj = -1;
          for (int cv = vlo; cv <= vhi; ++cv)
            for (int cu = ulo; cu <= uhi; ++cu) {                      // ascending rows: of equal d2 the first, the lowest row, stays
              const int j = cv * cam.W + cu;
              const float tx = target[(int64_t)j * 3], ty = target[(int64_t)j * 3 + 1], tz = target[(int64_t)j * 3 + 2];
              const float nx = normals[(int64_t)j * 3], ny = normals[(int64_t)j * 3 + 1], nz = normals[(int64_t)j * 3 + 2];
              bool ok = icp_finite(tx) && icp_finite(ty) && icp_finite(tz) && icp_finite(nx) && icp_finite(ny) && icp_finite(nz);
              if (src_normals != nullptr) ok = ok && dot3(mx, my, mz, nx, ny, nz) >= min_cos;   // (a NaN product fails)
              const float d2 = sqdist3(px, py, pz, tx, ty, tz);
              if (ok && d2 < bd) { bd = d2; bj = j; qx = tx; qy = ty; qz = tz; }
            }
          if (bj >= 0 && bd <= max2) found = bj;
        }
      }
    }
    if (idx_out != nullptr) idx_out[k] = found;
  }
  icp_accumulate(found, px, py, pz, qx, qy, qz, normals, s_part, partial);
}

__global__ __launch_bounds__(ICP_BLOCK) void icp_solve_kernel(const double* __restrict__ partial, int slots,
                                                              IcpState* __restrict__ state, double* __restrict__ sums_out,
                                                              double min_pairs) {
  __shared__ double s_run[ICP_PARTS][ICP_SLOT];
  __shared__ double s_sum[ICP_SLOT];
  if (state->status != ICP_RUNNING) return;
  const int tid = threadIdx.x, c = tid & (ICP_SLOT - 1), part = tid / ICP_SLOT;
  const int per = (slots + ICP_PARTS - 1) / ICP_PARTS;
  const int beg = part * per, end = min(slots, beg + per);
  double v = 0.0;
  if (c < ICP_SUMS)
    for (int s = beg; s < end; ++s) v += partial[(int64_t)s * ICP_SLOT + c];    // ascending slot order inside a run
  s_run[part][c] = v;
  __syncthreads();
  if (tid < ICP_SUMS) {
    v = 0.0;
#pragma unroll
    for (int p = 0; p < ICP_PARTS; ++p) v += s_run[p][tid];                     // the runs in order
    s_sum[tid] = v;
    if (sums_out != nullptr) sums_out[tid] = v;
  }
  __syncthreads();
  if (tid != 0) return;

  const double pairs = s_sum[28];
  const int it = state->iteration;
  if (it < ICP_MAX_ITER) {
    state->history[it][0] = pairs;
    state->history[it][1] = pairs > 0.0 ? sqrt(s_sum[27] / pairs) : 0.0;
  }
  state->iteration = it + 1;
  if (pairs < min_pairs) { state->status = ICP_TOO_FEW; return; }

  double Hm[6][6], L[6][6], g[6];
  {
    int q = 0;
#pragma unroll
    for (int u = 0; u < 6; ++u) {
#pragma unroll
      for (int w = u; w < 6; ++w) { Hm[u][w] = s_sum[q]; Hm[w][u] = s_sum[q]; ++q; }
    }
  }
  double top = 0.0;
#pragma unroll
  for (int u = 0; u < 6; ++u) { g[u] = s_sum[21 + u]; top = fmax(top, Hm[u][u]); }
  const double floor_pivot = 1e-12 * top;
  bool degenerate = false;
#pragma unroll
  for (int u = 0; u < 6; ++u) {                    // Cholesky H = L L^T, row by row; the pivot is L[u][u]^2
    double d = Hm[u][u];
#pragma unroll
    for (int w = 0; w < u; ++w) d -= L[u][w] * L[u][w];
    if (!(d > floor_pivot)) degenerate = true;     // (a NaN pivot too)
    const double root = sqrt(degenerate ? 1.0 : d);
    L[u][u] = root;
#pragma unroll
    for (int r = u + 1; r < 6; ++r) {
      double s = Hm[r][u];
#pragma unroll
      for (int w = 0; w < u; ++w) s -= L[r][w] * L[u][w];
      L[r][u] = s / root;
    }
  }
  if (degenerate) { state->status = ICP_DEGENERATE; return; }
  double yv[6], xv[6];
#pragma unroll
  for (int u = 0; u < 6; ++u) {                    // L y = -g
    double s = -g[u];
#pragma unroll
    for (int w = 0; w < u; ++w) s -= L[u][w] * yv[w];
    yv[u] = s / L[u][u];
  }
#pragma unroll
  for (int u = 5; u >= 0; --u) {                   // L^T x = y
    double s = yv[u];
#pragma unroll
    for (int w = u + 1; w < 6; ++w) s -= L[w][u] * xv[w];
    xv[u] = s / L[u][u];
  }
  const double wx = xv[0], wy = xv[1], wz = xv[2];
  const double th2 = (wx * wx + wy * wy) + wz * wz, th = sqrt(th2);
  const double tr = sqrt((xv[3] * xv[3] + xv[4] * xv[4]) + xv[5] * xv[5]);
  double A, B;
  if (th < 1e-6) { A = 1.0 - th2 / 6.0; B = 0.5 - th2 / 24.0; } else { A = sin(th) / th; B = (1.0 - cos(th)) / th2; }
  const double w3[3] = {wx, wy, wz};
  const double K[3][3] = {{0.0, -wz, wy}, {wz, 0.0, -wx}, {-wy, wx, 0.0}};
  double R[3][3], T[12];
#pragma unroll
  for (int u = 0; u < 3; ++u) {
#pragma unroll
    for (int w = 0; w < 3; ++w) R[u][w] = ((u == w ? 1.0 : 0.0) + A * K[u][w]) + B * (w3[u] * w3[w] - (u == w ? th2 : 0.0));
  }
#pragma unroll
  for (int u = 0; u < 12; ++u) T[u] = state->pose[u];
#pragma unroll
  for (int u = 0; u < 3; ++u) {
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      double s = (R[u][0] * T[w] + R[u][1] * T[4 + w]) + R[u][2] * T[8 + w];
      if (w == 3) s += xv[3 + u];
      state->pose[u * 4 + w] = s;
    }
  }
  if (th < state->rot_eps && tr < state->trans_eps) state->status = ICP_CONVERGED;
  else if (it + 1 >= state->max_iter) state->status = ICP_MAX_ITER_REACHED;
}

// The hand-over of one state block between the levels of a coarse-to-fine registration: one thread.  A registration that ended
// CONVERGED or MAX_ITER runs on -- the pose and the history stay -- with `budget` more steps; every other status is left as it is.
__global__ void icp_continue_kernel(IcpState* __restrict__ state, int budget, int* __restrict__ mark) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  const int it = state->iteration, status = state->status;
  if (mark != nullptr) { mark[0] = it; mark[1] = status; }
  if (status == ICP_CONVERGED || status == ICP_MAX_ITER_REACHED) {
    state->status = ICP_RUNNING;
    state->max_iter = min(ICP_MAX_ITER, it + budget);
  }
}

}  // namespace

extern "C" int regnet_icp_state_continue(void* state, int64_t budget, int32_t* mark, void* stream) {
  if (budget < 1 || budget > ICP_MAX_ITER) return REGNET_ERR_SHAPE;
  if (!state) return REGNET_ERR_NULL;
  hipLaunchKernelGGL(icp_continue_kernel, dim3(1), dim3(1), 0, as_stream(stream), (IcpState*)state, (int)budget, (int*)mark);
  REGNET_LAUNCH_CHECK();
  return REGNET_OK;
}

extern "C" int64_t regnet_icp_state_bytes(void) { return (int64_t)sizeof(IcpState); }

extern "C" int64_t regnet_icp_workspace_bytes(int64_t N_target, int64_t N_source) {
  if (N_target < 0 || N_source < 0 || N_target > ICP_MAX_POINTS || N_source > ICP_MAX_POINTS) return -1;
  const int64_t slots = icp_slots(N_source);
  return grid_slab_bytes(N_target) + (slots > 0 ? slots : 1) * ICP_SLOT * (int64_t)sizeof(double);
}

extern "C" int regnet_icp_prepare_f32(const float* target_xyz, int64_t N_target, double max_dist, void* workspace, void* stream) {
  if (N_target < 0) return REGNET_ERR_SHAPE;
  if (N_target > ICP_MAX_POINTS || !icp_dist_ok(max_dist)) return REGNET_ERR_UNSUPPORTED;
  if (!workspace || (N_target > 0 && !target_xyz)) return REGNET_ERR_NULL;
  return build_grid(target_xyz, 0, 1, 3, 1, N_target, (float)max_dist, workspace, as_stream(stream));
}

extern "C" int regnet_icp_step_f32(const float* source_xyz, int64_t N_source, int64_t stride, const float* target_normals,
                                   int64_t N_target, void* state, double max_dist, int32_t* idx_out, double* sums_out,
                                   int64_t min_pairs, void* workspace, void* stream) {
  if (N_source < 0 || N_target < 0 || stride < 1 || min_pairs < 0) return REGNET_ERR_SHAPE;
  if (N_source > ICP_MAX_POINTS || N_target > ICP_MAX_POINTS || !icp_dist_ok(max_dist)) return REGNET_ERR_UNSUPPORTED;
  if (!state || !workspace || (N_source > 0 && !source_xyz) || (N_target > 0 && !target_normals)) return REGNET_ERR_NULL;
  hipStream_t st = as_stream(stream);
  if (stride > ICP_MAX_POINTS) stride = ICP_MAX_POINTS;        // (N_source <= 2^21: the same single visited row, and no overflow below)
  const int64_t rows = icp_rows(N_source, stride), slots = icp_slots(rows);
  double* partial = reinterpret_cast<double*>((char*)workspace + grid_slab_bytes(N_target));
  if (slots > 0) {
    hipLaunchKernelGGL(icp_correspond_kernel, dim3((unsigned)slots), dim3(ICP_BLOCK), 0, st, source_xyz,
                       (int)stride, (int)rows, target_normals, (int)N_target,
                       (const IcpState*)state, (float)max_dist, (float)(max_dist * max_dist), (const char*)workspace, (int*)idx_out,
                       partial);
    REGNET_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(icp_solve_kernel, dim3(1), dim3(ICP_BLOCK), 0, st, (const double*)partial, (int)slots, (IcpState*)state,
                     sums_out, (double)min_pairs);
  REGNET_LAUNCH_CHECK();
  return REGNET_OK;
}

extern "C" int64_t regnet_icp_projective_workspace_bytes(int64_t N_source) {
  if (N_source < 0 || N_source > ICP_MAX_POINTS) return -1;
  const int64_t slots = icp_slots(N_source);
  return (slots > 0 ? slots : 1) * ICP_SLOT * (int64_t)sizeof(double);
}

extern "C" int regnet_icp_step_projective_f32(const float* source_xyz, int64_t N_source, int64_t stride,
                                              const float* source_normals, const float* target_xyz, const float* target_normals,
                                              int64_t W, int64_t H, const double* intrinsics, int64_t window, void* state,
                                              double max_dist, double min_cos, int32_t* idx_out, double* sums_out,
                                              int64_t min_pairs, void* workspace, void* stream) {
  if (N_source < 0 || W < 1 || H < 1 || stride < 1 || min_pairs < 0 || window < 0 || window > 2) return REGNET_ERR_SHAPE;
  if (N_source > ICP_MAX_POINTS || W > ICP_MAX_POINTS || H > ICP_MAX_POINTS || W * H > ICP_MAX_POINTS || !icp_dist_ok(max_dist))
    return REGNET_ERR_UNSUPPORTED;
  if (!(min_cos <= 1.0)) return REGNET_ERR_UNSUPPORTED;        // (a NaN too)
  if (!intrinsics) return REGNET_ERR_NULL;
  if (!icp_dist_ok(intrinsics[0]) || !icp_dist_ok(intrinsics[1])) return REGNET_ERR_UNSUPPORTED;
  const bool gate = !(min_cos < -1.0);
  if (!state || !workspace || !target_xyz || !target_normals || (N_source > 0 && (!source_xyz || (gate && !source_normals))))
    return REGNET_ERR_NULL;
  hipStream_t st = as_stream(stream);
  if (stride > ICP_MAX_POINTS) stride = ICP_MAX_POINTS;        // (N_source <= 2^21: the same single visited row, and no overflow below)
  const int64_t rows = icp_rows(N_source, stride), slots = icp_slots(rows);
  double* partial = reinterpret_cast<double*>(workspace);
  if (slots > 0) {
    IcpCamera cam;
    cam.W = (int)W; cam.H = (int)H; cam.window = (int)window;
    cam.fx = (float)intrinsics[0]; cam.fy = (float)intrinsics[1]; cam.cx = (float)intrinsics[2]; cam.cy = (float)intrinsics[3];
    hipLaunchKernelGGL(icp_project_kernel, dim3((unsigned)slots), dim3(ICP_BLOCK), 0, st, source_xyz, (int)stride, (int)rows,
                       gate ? source_normals : (const float*)nullptr, target_xyz, target_normals, cam, (const IcpState*)state,
                       (float)(max_dist * max_dist), gate ? (float)min_cos : 0.f, (int*)idx_out, partial);
    REGNET_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(icp_solve_kernel, dim3(1), dim3(ICP_BLOCK), 0, st, (const double*)partial, (int)slots, (IcpState*)state,
                     sums_out, (double)min_pairs);
  REGNET_LAUNCH_CHECK();
  return REGNET_OK;
}
