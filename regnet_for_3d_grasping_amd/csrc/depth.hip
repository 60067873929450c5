// depth.hip -- a depth camera's frame on the device (gfx950): a 16-bit (or float32) depth image and an optional 8-bit colour
// image in, the organised cloud that ingest.crop_frame and table_plane.estimate_plane take out (depth_frame.py).
//
// The contract is DESIGN.md par. 5 "Depth frames" and include/regnet_hip.h.  Built with -ffp-contract=off: every product, sum,
// difference and the one division below is an individually rounded binary32 operation in the written order, so a numpy float32
// restatement (tests/depth_reference.py) gives the same bits.
//
//   * depth_fill_kernel: the histogram to zero and, in registered mode, the z-buffer to the bits of +inf.
//   * depth_points_kernel<mode, uint16 | float>: a 32 x 8 pixel tile per 256-thread workgroup.  The tile's depths with a
//     one-pixel halo are decoded ONCE into LDS (34 x 10 metres + validity codes), so the 8-neighbour tests of the edge filter read
//     LDS and every input pixel leaves HBM about once (the halo: 340 / 256).  Depth, range, edge filter, deprojection.  Modes
//     none / aligned finish here (colour through the 256-entry table in constant memory, status, histogram): one launch
//     after the one-workgroup fill of the histogram.
//     Registered mode leaves provisional rows and does the footprint atomicMin's into the colour camera's z-buffer.
//   * depth_colour_kernel (registered mode only): recomputes the projection through the same depth_project(), tests visibility
//     against the z-buffer, gathers the colour, finalises xyz / rgb / status and the histogram.
//   * depth_normals_kernel (regnet_depth_normals_f32): the normals of an organised cloud from its own pixel grid, a lane per
//     pixel: the cross product of the differences `step` pixels along the row and the column, neighbours across a depth jump
//     left out.  What registration's projective mode takes as the target's (and the source's) normals.
//   * depth_bilateral_kernel (regnet_depth_bilateral_f32): the edge-preserving smoothing of a float32 depth image before it is
//     tracked, the same 32 x 8 tile with a halo of `radius` pixels and the two weight tables staged in LDS; the weights are DATA
//     (evaluated in float64 by the caller), so no device transcendental decides a bit.
//   * depth_halve_kernel (regnet_depth_halve_f32): one level of the image pyramid, a lane per coarse pixel over its 2 x 2 block.
// The launches are ordered by the stream: no workgroup waits for another, no flags, no cooperative launch.  Integer atomics only
// (the z-buffer's unsigned min on float bits -- positive finite floats order as their bits -- and one histogram add per
// workgroup and code); everything else is a plain vector store.
#include "common.h"

namespace {

constexpr long long DP_MAX_PIXELS = 1ll << 21;      // ingest.MAX_FRAME_POINTS: 1920 x 1080 fits
constexpr long long DP_MAX_COLOUR = 1ll << 23;
constexpr int DP_TX = 32, DP_TY = 8;                // the pixel tile: a wave half is one 128-byte row of float32 depths
constexpr int DP_BLOCK = DP_TX * DP_TY;
constexpr int DP_HX = DP_TX + 2, DP_HY = DP_TY + 2; // with the halo
constexpr int DP_HALO = DP_HX * DP_HY;
constexpr int DP_CODES = 8;
constexpr unsigned DP_QNAN = 0x7FC00000u;
constexpr unsigned DP_INF = 0x7F800000u;

enum { DP_NONE = 0, DP_ALIGNED = 1, DP_REGISTERED = 2 };
enum { ST_NO_DEPTH = 0, ST_RANGE = 1, ST_EDGE = 2, ST_NEIGHBOURS = 3, ST_OUTSIDE = 4, ST_OCCLUDED = 5, ST_KEPT = 6 };
enum { LD_ABSENT = 0, LD_RANGE = 1, LD_VALID = 2 };   // a halo slot: no depth (or beyond the image), out of range, valid0

// LUT[i] = float32(i / 255.0): the division in float64, rounded once -- evaluated by the host compiler
#define DP_L1(i) (float)((double)(i) / 255.0)
#define DP_L4(i) DP_L1(i), DP_L1((i) + 1), DP_L1((i) + 2), DP_L1((i) + 3)
#define DP_L16(i) DP_L4(i), DP_L4((i) + 4), DP_L4((i) + 8), DP_L4((i) + 12)
#define DP_L64(i) DP_L16(i), DP_L16((i) + 16), DP_L16((i) + 32), DP_L16((i) + 48)
#define DP_L256 DP_L64(0), DP_L64(64), DP_L64(128), DP_L64(192)
__constant__ float c_depth_lut[256] = {DP_L256};
const float h_depth_lut[256] = {DP_L256};

struct DepthArgs {
  int W, H, Wc, Hc;
  float rfx, rfy, cx, cy, scale, lo, hi, t, margin;
  float fxc, fyc, cxc, cyc;
  float r[9], tr[3];
  int use_edge, k, splat, keep;
};

__device__ __forceinline__ float decode(uint16_t d, float scale, bool& has) {
  has = d != 0;
  return (float)d * scale;
}
__device__ __forceinline__ float decode(float d, float, bool& has) {
  has = __builtin_isfinite(d) && d > 0.0f;
  return d;
}

struct Projection {
  bool inside;
  int fu, fv;
  float zp;
};

// the depth camera's point in the colour camera: both passes of registered mode go through here, so they agree bit for bit
__device__ __forceinline__ Projection depth_project(const DepthArgs& a, float x, float y, float z) {
  Projection p;
  p.inside = false;
  p.fu = p.fv = 0;
  const float xp = affine3(a.r[0], a.r[1], a.r[2], a.tr[0], x, y, z);
  const float yp = affine3(a.r[3], a.r[4], a.r[5], a.tr[1], x, y, z);
  const float zp = affine3(a.r[6], a.r[7], a.r[8], a.tr[2], x, y, z);
  p.zp = zp;
  if (!(__builtin_isfinite(zp) && zp > 0.0f)) return p;
  const float uc = (__fdiv_rn(xp, zp) * a.fxc) + a.cxc;
  const float vc = (__fdiv_rn(yp, zp) * a.fyc) + a.cyc;
  const float fu = floorf(uc + 0.5f), fv = floorf(vc + 0.5f);
  if (fu >= 0.0f && fu < (float)a.Wc && fv >= 0.0f && fv < (float)a.Hc) {      // in float: a NaN fails
    p.inside = true;
    p.fu = (int)fu;
    p.fv = (int)fv;
  }
  return p;
}

// one integer atomic per workgroup and code; every thread of the workgroup calls it (s_hist zeroed, a barrier since)
__device__ __forceinline__ void depth_histogram(bool active, int code, int* s_hist, int32_t* __restrict__ counts) {
#pragma unroll
  for (int c = 0; c <= ST_KEPT; ++c) {
    const int n = __popcll(__ballot(active && code == c));
    if (lane_id() == 0 && n != 0) atomicAdd(&s_hist[c], n);
  }
  __syncthreads();
  if (threadIdx.x < DP_CODES) {
    const int n = s_hist[threadIdx.x];
    if (n != 0) atomicAdd(&counts[threadIdx.x], n);
  }
}

__device__ __forceinline__ void store3(float* __restrict__ dst, long long row, float a, float b, float c) {
  dst[row * 3 + 0] = a; dst[row * 3 + 1] = b; dst[row * 3 + 2] = c;
}

__global__ __launch_bounds__(DP_BLOCK) void depth_fill_kernel(uint4* __restrict__ zbuf, long long n16,
                                                              int32_t* __restrict__ counts) {
  const long long i = (long long)blockIdx.x * DP_BLOCK + threadIdx.x;
  if (i < n16) zbuf[i] = make_uint4(DP_INF, DP_INF, DP_INF, DP_INF);
  if (blockIdx.x == 0 && threadIdx.x < DP_CODES) counts[threadIdx.x] = 0;
}

template <int MODE, typename D>
__global__ __launch_bounds__(DP_BLOCK) void depth_points_kernel(const D* __restrict__ depth, const uint8_t* __restrict__ colour,
                                                                const DepthArgs a, int tiles_x, float* __restrict__ xyz,
                                                                float* __restrict__ rgb, uint8_t* __restrict__ status,
                                                                int32_t* __restrict__ counts, unsigned* __restrict__ zbuf) {
  __shared__ float s_z[DP_HALO];
  __shared__ uint8_t s_code[DP_HALO];
  __shared__ int s_hist[DP_CODES];
  const int tid = threadIdx.x;
  const int u0 = (int)(blockIdx.x % (unsigned)tiles_x) * DP_TX, v0 = (int)(blockIdx.x / (unsigned)tiles_x) * DP_TY;
  if (tid < DP_CODES) s_hist[tid] = 0;
  for (int i = tid; i < DP_HALO; i += DP_BLOCK) {
    const int gu = u0 + i % DP_HX - 1, gv = v0 + i / DP_HX - 1;
    float z = 0.0f;
    int code = LD_ABSENT;
    if (gu >= 0 && gu < a.W && gv >= 0 && gv < a.H) {
      bool has;
      z = decode(depth[(long long)gv * a.W + gu], a.scale, has);
      if (has) code = (a.lo <= z && z <= a.hi) ? LD_VALID : LD_RANGE;
    }
    s_z[i] = z;
    s_code[i] = (uint8_t)code;
  }
  __syncthreads();
  const int lx = tid % DP_TX, ly = tid / DP_TX;
  const int u = u0 + lx, v = v0 + ly;
  const bool active = u < a.W && v < a.H;
  const long long row = (long long)v * a.W + u;
  int st = ST_NO_DEPTH;
  if (active) {
    const int at = (ly + 1) * DP_HX + lx + 1;
    const float z = s_z[at];
    const int own = s_code[at];
    st = own == LD_ABSENT ? ST_NO_DEPTH : (own == LD_RANGE ? ST_RANGE : ST_KEPT);
    if (st == ST_KEPT) {
      int neighbours = 0;
      bool jump = false;
#pragma unroll
      for (int dy = -1; dy <= 1; ++dy) {
#pragma unroll
        for (int dx = -1; dx <= 1; ++dx) {
          if (dx == 0 && dy == 0) continue;
          const int q = at + dy * DP_HX + dx;
          if (s_code[q] == LD_VALID) {
            ++neighbours;
            const float zq = s_z[q];
            const float e = a.t * fminf(z, zq);
            jump = jump || (fabsf(z - zq) > e);
          }
        }
      }
      if (a.use_edge && jump) st = ST_EDGE;
      else if (neighbours < a.k) st = ST_NEIGHBOURS;
    }
    const float nan = __uint_as_float(DP_QNAN);
    float x = nan, y = nan, zo = nan;
    if (st == ST_KEPT) {
      x = (((float)u - a.cx) * z) * a.rfx;
      y = (((float)v - a.cy) * z) * a.rfy;
      zo = z;
    }
    store3(xyz, row, x, y, zo);
    status[row] = (uint8_t)st;
    if (MODE == DP_REGISTERED) {
      if (st == ST_KEPT) {
        const Projection p = depth_project(a, x, y, zo);
        if (p.inside) {
          const unsigned bits = __float_as_uint(p.zp);
          const int ulo = max(p.fu - a.splat, 0), uhi = min(p.fu + a.splat, a.Wc - 1);
          const int vlo = max(p.fv - a.splat, 0), vhi = min(p.fv + a.splat, a.Hc - 1);
          for (int fv = vlo; fv <= vhi; ++fv)
            for (int fu = ulo; fu <= uhi; ++fu) atomicMin(&zbuf[(long long)fv * a.Wc + fu], bits);
        }
      }
    } else {
      float cr = 0.0f, cg = 0.0f, cb = 0.0f;
      if (MODE == DP_ALIGNED && st == ST_KEPT) {
        cr = c_depth_lut[colour[row * 3 + 0]]; cg = c_depth_lut[colour[row * 3 + 1]]; cb = c_depth_lut[colour[row * 3 + 2]];
      }
      store3(rgb, row, cr, cg, cb);
    }
  }
  if (MODE != DP_REGISTERED) depth_histogram(active, st, s_hist, counts);
}

__global__ __launch_bounds__(DP_BLOCK) void depth_colour_kernel(const uint8_t* __restrict__ colour, const DepthArgs a,
                                                                long long n, const unsigned* __restrict__ zbuf,
                                                                float* __restrict__ xyz, float* __restrict__ rgb,
                                                                uint8_t* __restrict__ status, int32_t* __restrict__ counts) {
  __shared__ int s_hist[DP_CODES];
  if (threadIdx.x < DP_CODES) s_hist[threadIdx.x] = 0;
  __syncthreads();
  const long long row = (long long)blockIdx.x * DP_BLOCK + threadIdx.x;
  const bool active = row < n;
  int st = ST_NO_DEPTH;
  if (active) {
    st = status[row];
    float cr = 0.0f, cg = 0.0f, cb = 0.0f;
    if (st == ST_KEPT) {
      const Projection p = depth_project(a, xyz[row * 3 + 0], xyz[row * 3 + 1], xyz[row * 3 + 2]);
      if (!p.inside) {
        st = ST_OUTSIDE;
      } else {
        const long long pix = (long long)p.fv * a.Wc + p.fu;
        const float zmin = __uint_as_float(zbuf[pix]);
        if (p.zp - zmin <= a.margin) {
          cr = c_depth_lut[colour[pix * 3 + 0]]; cg = c_depth_lut[colour[pix * 3 + 1]]; cb = c_depth_lut[colour[pix * 3 + 2]];
        } else {
          st = ST_OCCLUDED;
        }
      }
      if (st != ST_KEPT) {
        status[row] = (uint8_t)st;
        if (!a.keep) {
          const float nan = __uint_as_float(DP_QNAN);
          store3(xyz, row, nan, nan, nan);
        }
      }
    }
    store3(rgb, row, cr, cg, cb);
  }
  depth_histogram(active, st, s_hist, counts);
}

// one neighbour of the normal's difference: inside the image, finite, and within the jump of the centre's depth
__device__ __forceinline__ bool depth_neighbour(const float* __restrict__ xyz, int W, int H, int u, int v, float zc, float jump,
                                                float& x, float& y, float& z) {
  if (u < 0 || u >= W || v < 0 || v >= H) return false;
  const long long row = (long long)v * W + u;
  x = xyz[row * 3 + 0]; y = xyz[row * 3 + 1]; z = xyz[row * 3 + 2];
  return __builtin_isfinite(x) && __builtin_isfinite(y) && __builtin_isfinite(z) && fabsf(z - zc) <= jump;
}

// the difference along one image axis: far minus near when both neighbours are valid, else the valid one against the centre
__device__ __forceinline__ bool depth_difference(const float* __restrict__ xyz, int W, int H, int u, int v, int du, int dv,
                                                 float cx, float cy, float cz, float jump, float& dx, float& dy, float& dz) {
  float ax = 0.0f, ay = 0.0f, az = 0.0f, bx = 0.0f, by = 0.0f, bz = 0.0f;
  const bool near = depth_neighbour(xyz, W, H, u - du, v - dv, cz, jump, ax, ay, az);
  const bool far = depth_neighbour(xyz, W, H, u + du, v + dv, cz, jump, bx, by, bz);
  if (!near && !far) return false;
  if (!near) { ax = cx; ay = cy; az = cz; }
  if (!far) { bx = cx; by = cy; bz = cz; }
  dx = bx - ax; dy = by - ay; dz = bz - az;
  return true;
}

// depth_normals_kernel: a lane per pixel of an organised cloud; the normal is the cross product of the differences along the
// image row and column, scaled to length 1 and turned to face the camera at the origin.  No normal: three NaNs.
__global__ __launch_bounds__(DP_BLOCK) void depth_normals_kernel(const float* __restrict__ xyz, int W, int H, int step, float jump,
                                                                 float* __restrict__ normals) {
  const long long row = (long long)blockIdx.x * DP_BLOCK + threadIdx.x;
  if (row >= (long long)W * H) return;
  const int u = (int)(row % W), v = (int)(row / W);
  const float nan = __uint_as_float(DP_QNAN);
  float nx = nan, ny = nan, nz = nan;
  const float cx = xyz[row * 3 + 0], cy = xyz[row * 3 + 1], cz = xyz[row * 3 + 2];
  float hx, hy, hz, gx, gy, gz;
  if (__builtin_isfinite(cx) && __builtin_isfinite(cy) && __builtin_isfinite(cz) &&
      depth_difference(xyz, W, H, u, v, step, 0, cx, cy, cz, jump, hx, hy, hz) &&
      depth_difference(xyz, W, H, u, v, 0, step, cx, cy, cz, jump, gx, gy, gz)) {
    const float ax = (hy * gz) - (hz * gy), ay = (hz * gx) - (hx * gz), az = (hx * gy) - (hy * gx);
    const float len2 = ((ax * ax) + (ay * ay)) + (az * az);
    if (__builtin_isfinite(len2) && len2 > 0.0f) {
      const float len = sqrtf(len2);      // correctly rounded (this toolchain's __fsqrt_rn is the native approximation, an ulp off)
      nx = __fdiv_rn(ax, len); ny = __fdiv_rn(ay, len); nz = __fdiv_rn(az, len);
      if (((nx * cx) + (ny * cy)) + (nz * cz) > 0.0f) { nx = -nx; ny = -ny; nz = -nz; }
    }
  }
  store3(normals, row, nx, ny, nz);
}

// ---- smoothing and the pyramid (regnet_depth_bilateral_f32, regnet_depth_halve_f32) ------------------------------------------
constexpr int DB_MAX_RADIUS = 4;
constexpr int DB_RANGE = 256;                                                     // entries of the range table
constexpr int DB_MAX_HALO = (DP_TX + 2 * DB_MAX_RADIUS) * (DP_TY + 2 * DB_MAX_RADIUS);
constexpr int DB_MAX_TABLES = (2 * DB_MAX_RADIUS + 1) * (2 * DB_MAX_RADIUS + 1) + DB_RANGE;

__device__ __forceinline__ bool depth_has(float z) { return __builtin_isfinite(z) && z > 0.0f; }

// depth_bilateral_kernel: a lane per pixel of a 32 x 8 tile.  The tile's depths with a halo of `radius` pixels go to LDS once,
// "no depth" and "beyond the image" as NaN, and so do the (2 radius + 1)^2 spatial weights and the 256 range weights; the
// window then reads LDS only.  The sums run b outer, a inner, the centre in its place: the written order of the contract.
__global__ __launch_bounds__(DP_BLOCK) void depth_bilateral_kernel(const float* __restrict__ depth, int W, int H, int radius,
                                                                   const float* __restrict__ tables, float rbin, int tiles_x,
                                                                   float* __restrict__ out) {
  __shared__ float s_z[DB_MAX_HALO];
  __shared__ float s_t[DB_MAX_TABLES];
  const int tid = threadIdx.x;
  const int side = 2 * radius + 1, hx = DP_TX + 2 * radius, halo = hx * (DP_TY + 2 * radius), n_tables = side * side + DB_RANGE;
  const int u0 = (int)(blockIdx.x % (unsigned)tiles_x) * DP_TX, v0 = (int)(blockIdx.x / (unsigned)tiles_x) * DP_TY;
  const float nan = __uint_as_float(DP_QNAN);
  for (int i = tid; i < halo; i += DP_BLOCK) {
    const int gu = u0 + i % hx - radius, gv = v0 + i / hx - radius;
    float z = nan;
    if (gu >= 0 && gu < W && gv >= 0 && gv < H) {
      const float d = depth[(long long)gv * W + gu];
      if (depth_has(d)) z = d;
    }
    s_z[i] = z;
  }
  for (int i = tid; i < n_tables; i += DP_BLOCK) s_t[i] = tables[i];
  __syncthreads();
  const int lx = tid % DP_TX, ly = tid / DP_TX;
  const int u = u0 + lx, v = v0 + ly;
  if (u >= W || v >= H) return;
  const int at = (ly + radius) * hx + lx + radius;
  const float zc = s_z[at];
  float result = nan;
  if (zc == zc) {                                             // a valid centre (LDS holds NaN for every other kind)
    const float* range = s_t + side * side;
    float sw = 0.0f, sd = 0.0f;
    for (int b = -radius; b <= radius; ++b)
      for (int a = -radius; a <= radius; ++a) {
        const float zq = s_z[at + b * hx + a];
        if (!(zq == zq)) continue;
        const float d = zq - zc;
        const float t = fabsf(d) * rbin;
        if (!(t < (float)DB_RANGE)) continue;                 // beyond three sigma: no weight at all
        const float w = s_t[(b + radius) * side + (a + radius)] * range[(int)t];
        sw = sw + w;
        sd = sd + (w * d);
      }
    result = zc + __fdiv_rn(sd, sw);                          // (the centre gave S[0][0] G[0] > 0)
  }
  out[(long long)v * W + u] = result;
}

// depth_halve_kernel: a lane per coarse pixel; its block (2u, 2v), (2u+1, 2v), (2u, 2v+1), (2u+1, 2v+1) in that order.
__global__ __launch_bounds__(DP_BLOCK) void depth_halve_kernel(const float* __restrict__ depth, int W, int Wo, long long n_out,
                                                               float cutoff, float* __restrict__ out) {
  const long long row = (long long)blockIdx.x * DP_BLOCK + threadIdx.x;
  if (row >= n_out) return;
  const int u = (int)(row % Wo), v = (int)(row / Wo);
  const float* top = depth + (long long)(2 * v) * W + 2 * u;  // (scalar loads: with an odd W the lower row is not 8-byte aligned)
  const float z[4] = {top[0], top[1], top[W], top[W + 1]};
  float ref = __builtin_inff();
#pragma unroll
  for (int k = 0; k < 4; ++k)
    if (depth_has(z[k]) && z[k] < ref) ref = z[k];
  float sum = 0.0f;
  int count = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k)
    if (depth_has(z[k]) && z[k] - ref <= cutoff) { sum = sum + z[k]; ++count; }
  out[row] = count > 0 ? __fdiv_rn(sum, (float)count) : __uint_as_float(DP_QNAN);
}

int depth_check(int64_t W, int64_t H, int64_t Wc, int64_t Hc, int mode) {
  if (W < 1 || H < 1 || mode < DP_NONE || mode > DP_REGISTERED) return REGNET_ERR_SHAPE;
  if (mode == DP_ALIGNED && (Wc != W || Hc != H)) return REGNET_ERR_SHAPE;
  if (mode == DP_REGISTERED && (Wc < 1 || Hc < 1)) return REGNET_ERR_SHAPE;
  if (W > DP_MAX_PIXELS || H > DP_MAX_PIXELS || W * H > DP_MAX_PIXELS) return REGNET_ERR_UNSUPPORTED;
  if (mode == DP_REGISTERED && (Wc > DP_MAX_COLOUR || Hc > DP_MAX_COLOUR || Wc * Hc > DP_MAX_COLOUR)) return REGNET_ERR_UNSUPPORTED;
  return REGNET_OK;
}

template <typename D>
int depth_launch(const D* depth, int64_t W, int64_t H, const float* params, const uint8_t* colour, int64_t Wc, int64_t Hc,
                 int mode, int use_edge, int min_neighbours, int splat, int keep_uncoloured, float* xyz, float* rgb,
                 uint8_t* status, int32_t* counts, void* workspace, void* stream) {
  const int bad = depth_check(W, H, Wc, Hc, mode);
  if (bad == REGNET_ERR_SHAPE) return bad;
  if (min_neighbours < 0 || min_neighbours > 8 || splat < 0 || splat > 2) return REGNET_ERR_SHAPE;
  if (bad != REGNET_OK) return bad;
  if (!depth || !params || !xyz || !rgb || !status || !counts) return REGNET_ERR_NULL;
  if (mode != DP_NONE && !colour) return REGNET_ERR_NULL;
  if (mode == DP_REGISTERED && !workspace) return REGNET_ERR_NULL;
  hipStream_t s = as_stream(stream);
  DepthArgs a;
  a.W = (int)W; a.H = (int)H;
  a.Wc = mode == DP_REGISTERED ? (int)Wc : 0; a.Hc = mode == DP_REGISTERED ? (int)Hc : 0;
  a.rfx = params[0]; a.rfy = params[1]; a.cx = params[2]; a.cy = params[3]; a.scale = params[4];
  a.lo = params[5]; a.hi = params[6]; a.t = params[7]; a.margin = params[8];
  a.fxc = params[9]; a.fyc = params[10]; a.cxc = params[11]; a.cyc = params[12];
  for (int i = 0; i < 9; ++i) a.r[i] = params[13 + i];
  for (int i = 0; i < 3; ++i) a.tr[i] = params[22 + i];
  a.use_edge = use_edge ? 1 : 0; a.k = min_neighbours; a.splat = splat; a.keep = keep_uncoloured ? 1 : 0;
  const int tiles_x = (int)((W + DP_TX - 1) / DP_TX), tiles_y = (int)((H + DP_TY - 1) / DP_TY);
  const dim3 grid((unsigned)(tiles_x * tiles_y)), block(DP_BLOCK);
  const long long n = (long long)(W * H);
  if (mode == DP_REGISTERED) {
    const long long n16 = ((long long)(Wc * Hc) * 4 + 15) / 16;
    hipLaunchKernelGGL(depth_fill_kernel, dim3((unsigned)((n16 + DP_BLOCK - 1) / DP_BLOCK)), block, 0, s, (uint4*)workspace, n16,
                       counts);
    REGNET_LAUNCH_CHECK();
    hipLaunchKernelGGL((depth_points_kernel<DP_REGISTERED, D>), grid, block, 0, s, depth, colour, a, tiles_x, xyz, rgb, status,
                       counts, (unsigned*)workspace);
    REGNET_LAUNCH_CHECK();
    hipLaunchKernelGGL(depth_colour_kernel, dim3((unsigned)((n + DP_BLOCK - 1) / DP_BLOCK)), block, 0, s, colour, a, n,
                       (const unsigned*)workspace, xyz, rgb, status, counts);
    REGNET_LAUNCH_CHECK();
    return REGNET_OK;
  }
  // (a kernel and not a 32-byte memset: the call stays one chain of kernel nodes when it is captured into a graph)
  hipLaunchKernelGGL(depth_fill_kernel, dim3(1), block, 0, s, (uint4*)nullptr, 0ll, counts);
  REGNET_LAUNCH_CHECK();
  if (mode == DP_ALIGNED) {
    hipLaunchKernelGGL((depth_points_kernel<DP_ALIGNED, D>), grid, block, 0, s, depth, colour, a, tiles_x, xyz, rgb, status, counts,
                       (unsigned*)nullptr);
  } else {
    hipLaunchKernelGGL((depth_points_kernel<DP_NONE, D>), grid, block, 0, s, depth, colour, a, tiles_x, xyz, rgb, status, counts,
                       (unsigned*)nullptr);
  }
  REGNET_LAUNCH_CHECK();
  return REGNET_OK;
}

}  // namespace

extern "C" int64_t regnet_depth_workspace_bytes(int64_t W, int64_t H, int64_t Wc, int64_t Hc, int mode) {
  if (depth_check(W, H, Wc, Hc, mode) != REGNET_OK) return -1;
  return mode == DP_REGISTERED ? (Wc * Hc * 4 + 15) / 16 * 16 : 16;
}

extern "C" int regnet_depth_colour_lut(float* lut) {
  if (!lut) return REGNET_ERR_NULL;
  for (int i = 0; i < 256; ++i) lut[i] = h_depth_lut[i];
  return REGNET_OK;
}

extern "C" int regnet_depth_to_cloud_u16(const uint16_t* depth, int64_t W, int64_t H, const float* params, const uint8_t* colour,
                                         int64_t Wc, int64_t Hc, int mode, int use_edge, int min_neighbours, int splat,
                                         int keep_uncoloured, float* xyz, float* rgb, uint8_t* status, int32_t* counts,
                                         void* workspace, void* stream) {
  return depth_launch<uint16_t>(depth, W, H, params, colour, Wc, Hc, mode, use_edge, min_neighbours, splat, keep_uncoloured, xyz,
                                rgb, status, counts, workspace, stream);
}

extern "C" int regnet_depth_to_cloud_f32(const float* depth, int64_t W, int64_t H, const float* params, const uint8_t* colour,
                                         int64_t Wc, int64_t Hc, int mode, int use_edge, int min_neighbours, int splat,
                                         int keep_uncoloured, float* xyz, float* rgb, uint8_t* status, int32_t* counts,
                                         void* workspace, void* stream) {
  return depth_launch<float>(depth, W, H, params, colour, Wc, Hc, mode, use_edge, min_neighbours, splat, keep_uncoloured, xyz, rgb,
                             status, counts, workspace, stream);
}

extern "C" int regnet_depth_normals_f32(const float* xyz, int64_t W, int64_t H, int64_t step, double max_jump, float* normals,
                                        void* stream) {
  if (W < 1 || H < 1 || step < 1) return REGNET_ERR_SHAPE;
  if (W > DP_MAX_PIXELS || H > DP_MAX_PIXELS || W * H > DP_MAX_PIXELS) return REGNET_ERR_UNSUPPORTED;
  const float jump = (float)max_jump;
  if (!(max_jump > 0.0 && jump > 0.0f && jump < __builtin_inff())) return REGNET_ERR_UNSUPPORTED;   // (a NaN too)
  if (!xyz || !normals) return REGNET_ERR_NULL;
  if (step > DP_MAX_PIXELS) step = DP_MAX_PIXELS;      // (beyond the image either way, and no overflow in u + step)
  const long long n = (long long)(W * H);
  hipLaunchKernelGGL(depth_normals_kernel, dim3((unsigned)((n + DP_BLOCK - 1) / DP_BLOCK)), dim3(DP_BLOCK), 0, as_stream(stream),
                     xyz, (int)W, (int)H, (int)step, jump, normals);
  REGNET_LAUNCH_CHECK();
  return REGNET_OK;
}

extern "C" int regnet_depth_bilateral_f32(const float* depth, int64_t W, int64_t H, int64_t radius, const float* tables, double rbin,
                                          float* out, void* stream) {
  if (W < 1 || H < 1 || radius < 1 || radius > DB_MAX_RADIUS) return REGNET_ERR_SHAPE;
  if (W > DP_MAX_PIXELS || H > DP_MAX_PIXELS || W * H > DP_MAX_PIXELS) return REGNET_ERR_UNSUPPORTED;
  const float bin = (float)rbin;
  if (!(rbin > 0.0 && bin > 0.0f && bin < __builtin_inff())) return REGNET_ERR_UNSUPPORTED;           // (a NaN too)
  if (!depth || !tables || !out) return REGNET_ERR_NULL;
  const int tiles_x = (int)((W + DP_TX - 1) / DP_TX), tiles_y = (int)((H + DP_TY - 1) / DP_TY);
  hipLaunchKernelGGL(depth_bilateral_kernel, dim3((unsigned)(tiles_x * tiles_y)), dim3(DP_BLOCK), 0, as_stream(stream), depth,
                     (int)W, (int)H, (int)radius, tables, bin, tiles_x, out);
  REGNET_LAUNCH_CHECK();
  return REGNET_OK;
}

extern "C" int regnet_depth_halve_f32(const float* depth, int64_t W, int64_t H, double cutoff, float* out, void* stream) {
  if (W < 2 || H < 2) return REGNET_ERR_SHAPE;
  if (W > DP_MAX_PIXELS || H > DP_MAX_PIXELS || W * H > DP_MAX_PIXELS) return REGNET_ERR_UNSUPPORTED;
  const float cut = (float)cutoff;
  if (!(cutoff > 0.0 && cut > 0.0f && cut < __builtin_inff())) return REGNET_ERR_UNSUPPORTED;         // (a NaN too)
  if (!depth || !out) return REGNET_ERR_NULL;
  const int64_t Wo = W / 2, Ho = H / 2;
  const long long n = (long long)(Wo * Ho);
  hipLaunchKernelGGL(depth_halve_kernel, dim3((unsigned)((n + DP_BLOCK - 1) / DP_BLOCK)), dim3(DP_BLOCK), 0, as_stream(stream),
                     depth, (int)W, (int)Wo, n, cut, out);
  REGNET_LAUNCH_CHECK();
  return REGNET_OK;
}
