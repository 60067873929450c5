// scatter_plan.h -- layout of the per-scene sort plan of the deterministic scatter-adds (built by ops_f64.hip, read by the
// float64 segment sums there and the float32 ones of det.hip).
//
// Per scene: R destinations, L sources (flattened source position p, index[b, p] its destination).  The plan is
//   cursor int32[B*R]      -- scratch of the placement,
//   offset int32[B*(R+1)]  -- segment of destination n: [offset[n], offset[n+1]),
//   perm   int32[B*L]      -- the source positions of every segment, ascending.
// Sources whose index lies outside [0, R) are in no segment.
#pragma once
#include <stdint.h>

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
