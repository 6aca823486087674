// Tiny-splat backward: slab addressing shared by both passes, and pass 2, which runs inside the projection backward
// (fused_project_bwd.hip: k_fproject_bwd).  raster_px.hip has pass 1 (k_tiny_bwd) and the story.
#pragma once
#include "gsloc_common.h"

namespace gsl {

__device__ __forceinline__ int tiny_origin(float centre, float r) {  // first pixel index within r of centre
  return (int)ceilf(centre - r - 0.5f);
}

// Lane r (0..3) of a quad folds row r of Gaussian gid's 4x4 slab of (w, alpha*T) records into the gradient row
// [v_xy 2 | v_conic 3 | v_opacity 1 | v_colour D] (dx, dy rebuilt from the Gaussian's own record), clears the slab row,
// and the quad's four partial rows are added up: every lane of the quad returns the Gaussian's total.
// Split in two (round 4): tiny_slab_load issues every load that does not depend on another one -- radius, the slab row,
// both records -- and tiny_slab_fold works on them; the caller loads two items, consumes all loads at once (empty asm) and
// folds.  Written as one function called four times in a rolled loop, a thread went through radius -> slab -> records ->
// upstream pixels four times in a row: sixteen dependent memory round trips, half of the projection backward's 16 us in a
// tracker iteration at 102 k Gaussians.
struct TinySlabIn {
  int rad;
  float4 lo, hi, q0, qc;
};
__device__ __forceinline__ TinySlabIn tiny_slab_load(const int32_t* __restrict__ radii, const float4* __restrict__ Q0,
                                                     const float4* __restrict__ Q1, const float4* __restrict__ trec,
                                                     int gid, int r, int N) {
  TinySlabIn in;
  const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
  in.rad = 0; in.lo = z; in.hi = z; in.q0 = z; in.qc = z;
  if (gid < N) {
    const float4* row = trec + (size_t)gid * 8 + 2 * r;  // slab = 16 float2 = 8 float4; row r = float4 2r, 2r+1
    in.rad = radii[gid];
    in.lo = row[0];
    in.hi = row[1];
    in.q0 = Q0[gid];
    in.qc = Q1[gid];
  }
  return in;
}
#define GSL_TINY_SLAB_PIN(in)                                                                                         \
  asm volatile("" : "+v"((in).rad), "+v"((in).lo.x), "+v"((in).lo.y), "+v"((in).lo.z), "+v"((in).lo.w), "+v"((in).hi.x), \
               "+v"((in).hi.y), "+v"((in).hi.z), "+v"((in).hi.w), "+v"((in).q0.x), "+v"((in).q0.y), "+v"((in).q0.z),    \
               "+v"((in).q0.w), "+v"((in).qc.x), "+v"((in).qc.y), "+v"((in).qc.z), "+v"((in).qc.w)                       \
               :                                                                                                      \
               : "memory")
template <int D>
__device__ __forceinline__ void tiny_slab_fold(const TinySlabIn& in, int W, int H, float4* __restrict__ trec,
                                               const float* __restrict__ vcT, int gid, int r, float (&v)[6 + D]) {
  constexpr int A = 6 + D;
#pragma unroll
  for (int k = 0; k < A; ++k) v[k] = 0.f;
  if (in.rad > 0) {
    float4* row = trec + (size_t)gid * 8 + 2 * r;
    const float4 lo = in.lo, hi = in.hi;
    float w[4] = {lo.x, lo.z, hi.x, hi.z}, f[4] = {lo.y, lo.w, hi.y, hi.w};
    bool any = false;
#pragma unroll
    for (int c = 0; c < 4; ++c) any = any || (w[c] != 0.f) || (f[c] != 0.f);
    if (any) {
      float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
      row[0] = z;
      row[1] = z;
      const float4 q0 = in.q0, qc = in.qc;
      int pcol0 = tiny_origin(q0.x, qc.w), prow = tiny_origin(q0.y, qc.w) + r;
      float dy = q0.y - ((float)prow + 0.5f);
      bool row_in = (unsigned)prow < (unsigned)H;
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        if (w[c] != 0.f || f[c] != 0.f) {
          int pcol = pcol0 + c;
          float dx = q0.x - ((float)pcol + 0.5f);
          float gx = qc.x * dx + qc.y * dy, gy = qc.y * dx + qc.z * dy;
          float v_sigma = -q0.w * w[c], hs = 0.5f * v_sigma;
          v[0] += v_sigma * gx; v[1] += v_sigma * gy;
          v[2] += hs * dx * dx; v[3] += v_sigma * dx * dy; v[4] += hs * dy * dy;
          v[5] += w[c];
          if (f[c] != 0.f && row_in && (unsigned)pcol < (unsigned)W) {
            size_t pid = (size_t)prow * W + pcol;
#pragma unroll
            for (int k = 0; k < D; ++k) v[6 + k] += f[c] * vcT[pid * D + k];
          }
        }
      }
    }
  }
#pragma unroll
  for (int k = 0; k < A; ++k) {
    float x = v[k];
    x += dpp_get<0xB1>(x);  // quad_perm [1,0,3,2]
    x += dpp_get<0x4E>(x);  // quad_perm [2,3,0,1]: every lane of the quad holds the Gaussian's total
    v[k] = x;
  }
}

}  // namespace gsl
