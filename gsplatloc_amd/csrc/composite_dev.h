// The steps every compositing kernel opens (or closes) with, once: the tile's list span, the lane -> pixel maps, the
// backward's per-pixel starting state, the trim of the list to the last composited entry, the clearing of the tile
// counters, the fused forward's alpha expression, the colour dot and the forward's pixel write-out.  Used by
// raster_px.hip (k_praster_fwd, k_long_fwd, k_long_combine, k_tiny_bwd), raster_g16.hip (qraster_bwd_item / _body),
// raster_det.hip (k_mraster_bwd), absgrad.hip (k_absgrad) and raster.hip (k_raster_fwd / k_raster_bwd).  The walks
// themselves are scheduled by hand per kernel and stay where they are.  Every helper is forced inline and does what the
// hand-written copies did, in their order.  The bar: no kernel costs a register, an LDS byte or a wave more than with its
// own copy (NOTES.md has the table; tests/test_kernel_resources.py pins it).  Two kernels miss it with one helper each and
// keep that step written out: see the notes at bwd_start and clear_tile_counter.
#pragma once
#include "long_dev.h"

namespace gsl {

// ---- 1. the tile's span of the sorted list -----------------------------------------------------------------------------
struct ListSpan {
  long long rs, re;  // [rs, re) of flatten_ids
};
// tile_offsets[tile] .. tile_offsets[tile + 1], the end clamped to the capacity of the list (what did not fit was never
// written; the total tells the host)
__device__ __forceinline__ ListSpan tile_span(const int32_t* tile_offsets, int tile, long long capacity) {
  ListSpan s{tile_offsets[tile], tile_offsets[tile + 1]};
  if (s.re > capacity) s.re = capacity;
  return s;
}
// segment sgm (GSL_SEG entries, long_dev.h) of a long tile's span
__device__ __forceinline__ ListSpan segment_span(ListSpan tile, int sgm) {
  const long long ss = tile.rs + (long long)sgm * GSL_SEG;
  return {ss, min(ss + (long long)GSL_SEG, tile.re)};
}

// ---- 2. lane -> pixel: a wave owns one 8x8 quadrant of a 16x16 tile --------------------------------------------------------
struct TilePixel {
  int tyi, txi, qx, qy, i, j;  // tile coordinates, the quadrant's first pixel, the lane's pixel (row i, column j)
  float px, py;                // ... and its centre
};
// BLOCKS: DPP row g of the wave = 4x4 block g of the quadrant, lane p of the row = pixel (p & 3, p >> 2) of the block (the
// fused forward and the general backward: a per-block reduction is then a row reduction); else lane = 8 y + x
template <bool BLOCKS>
__device__ __forceinline__ TilePixel quadrant_pixel(int tile, int tile_w, int quad, int lane) {
  TilePixel t;
  t.tyi = tile / tile_w;
  t.txi = tile - t.tyi * tile_w;
  t.qx = t.txi * 16 + (quad & 1) * 8;
  t.qy = t.tyi * 16 + (quad >> 1) * 8;
  if (BLOCKS) {
    const int grp = lane >> 4, pp = lane & 15;
    t.j = t.qx + 4 * (grp & 1) + (pp & 3);
    t.i = t.qy + 4 * (grp >> 1) + (pp >> 2);
  } else {
    t.j = t.qx + (lane & 7);
    t.i = t.qy + (lane >> 3);
  }
  t.px = (float)t.j + 0.5f;
  t.py = (float)t.i + 0.5f;
  return t;
}
// 256-thread workgroup per tile, wave tid >> 6 = quadrant, the block map (the row map: quadrant_pixel<false>(.., wv, lane))
__device__ __forceinline__ TilePixel tile_pixel(int tile, int tile_w, int tid) {
  return quadrant_pixel<true>(tile, tile_w, tid >> 6, tid & 63);
}
// inside the frame and the pixel rows [row0, row1) of the call (a whole-frame kernel passes 0, H)
__device__ __forceinline__ bool pixel_inside(const TilePixel& t, int W, int H, int row0, int row1) {
  return (t.i < H) && (t.j < W) && (t.i >= row0) && (t.i < row1);
}
// index into the [H, W] images; 0 for a lane without a pixel (it loads nothing)
__device__ __forceinline__ size_t pixel_index(const TilePixel& t, int W, bool inside) {
  return inside ? ((size_t)t.i * W + t.j) : 0;
}

// ---- 3. the backward's starting state of a pixel, in pieces: no kernel loads earlier than it has to ------------------------
// the last list entry the pixel composited (-1: none, or no pixel)
__device__ __forceinline__ int last_composited(const int32_t* last_ids, size_t pid, bool inside) {
  return inside ? last_ids[pid] : -1;
}
// the upstream colour gradient
template <int D>
__device__ __forceinline__ void load_upstream(const float* v_render, size_t pid, bool inside, float (&vc)[D]) {
#pragma unroll
  for (int k = 0; k < D; ++k) vc[k] = inside ? v_render[pid * D + k] : 0.f;
}
// the rest: the image's alpha, T behind the last entry, the alpha gradient with the expected-depth chain folded into it and
// into vc[D - 1] (ED; gsloc_common.h ed_backward), and -- formed where the caller starts its walk -- the walk's running
// sum  Bp = -T_final v_alpha  (v_alpha of an entry = T c.v - (sum behind it + Bp) / (1 - alpha)).  A background term is
// the caller's to add.
// k_tiny_bwd (raster_px.hip) keeps a copy of its own of this piece: with the call -- in one piece or split into loads and
// expected-depth chain, in whatever order around the LDS read of its loss gradient -- k_tiny_bwd<4, true, true>, the
// tracker's kernel, needs 71 VGPRs instead of 67 (the other eight instantiations are indifferent).
struct BwdStart {
  float Aimg, T_final, va;
  __device__ __forceinline__ float Bp() const { return -T_final * va; }
};
template <int D, bool ED>
__device__ __forceinline__ BwdStart bwd_start(const float* alphas, const float* render, const float* v_alphas, size_t pid,
                                              bool inside, float (&vc)[D]) {
  BwdStart s;
  s.Aimg = inside ? alphas[pid] : 0.f;
  s.T_final = 1.f - s.Aimg;
  s.va = inside ? v_alphas[pid] : 0.f;
  if (ED && inside) {
    const EdGrad g = ed_backward(s.Aimg, render[pid * D + (D - 1)], s.va, vc[D - 1]);
    s.va = g.va;
    vc[D - 1] = g.vd;
  }
  return s;
}

// ---- 4. nothing behind the last entry that a pixel of the wave / the tile composited is walked -----------------------------
__device__ __forceinline__ int wave_max(int v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v = max(v, __shfl_xor(v, o, 64));
  return v;
}
__device__ __forceinline__ void trim_span(ListSpan& s, int last) {
  if ((long long)last + 1 < s.re) s.re = max((long long)last + 1, s.rs);
}
// The tile's last entry from the four waves' (lane 0 of wave w has stored its wave_max in s_last[w]), and the trim.  The
// barrier between the stores and this is the CALLER's: each kernel has one there anyway (k_mraster_bwd its
// __syncthreads_or), and none is added here.
__device__ __forceinline__ void block_last_trim(const int (&s_last)[4], ListSpan& s) {
  trim_span(s, max(max(s_last[0], s_last[1]), max(s_last[2], s_last[3])));
}

// ---- 5. the tile counters of the binned projection are cleared by the compositing kernel that runs once they are consumed:
// the forward, or -- behind a forward that sorted its own tile bin (k_praster_fwd, SORT) while other workgroups were
// still adding the counters up -- the first kernel of the backward.  One thread per tile; the first workgroup clears the
// state word ("the next projection may bin").
// qraster_bwd_item (raster_g16.hip) keeps a copy of its own: k_qraster_bwd sits at the scalar-register limit (106 SGPRs,
// some already kept in VGPR lanes), and with the clearing behind a call -- its condition split in two, whichever way --
// every non-LONG instantiation needs 1 to 6 more VGPRs; k_qraster_bwd<3, false, 3, false> loses a wave per SIMD (80 -> 81).
__device__ __forceinline__ void clear_tile_counter(int32_t* __restrict__ clear_counts, int32_t* __restrict__ clear_state,
                                                   int tile, bool first) {
  if (clear_counts && threadIdx.x == 0) {
    clear_counts[tile] = 0;
    if (first && clear_state) *clear_state = 0;
  }
}

// ---- 6. alpha of the fused pipeline ------------------------------------------------------------------------------------
// The conic is staged times log2(e) with its diagonal halved, so that a trip gets  log2(e) sigma = a' dx^2 + c' dy^2 + b' dx dy
// in six operations and  alpha = opacity exp2(-that)  without the scaling multiply of expf.  The forward (praster_walk)
// and every backward that replays it (k_tiny_bwd, qraster_bwd_body, k_absgrad) call these two and nothing else: both sides
// evaluate alpha with the very same operations and take the same alpha >= 1/255 decision for every (pixel, entry) pair.
// The staged kernels (raster.hip) do not use this: k_raster_bwd pairs with k_raster_fwd, both of the __expf form.
// The deterministic backward (raster_det.hip, k_mraster_bwd) does not use it either, but it is NOT paired with a forward
// of its own form: a deterministic RenderContext runs praster_walk (exp2, staged conic) forward and k_mraster_bwd
// (__expf, plain conic) backward.  The two alphas differ in the last bits (a few 1e-7 relative), so on a (pixel, entry)
// pair whose alpha sits within that of 1/255 the backward can skip an entry the forward composited, or the reverse: T
// behind that entry is then off by the factor 1 - 1/255 in that pixel's gradient terms.  No test has met such a pair (the
// stop-ladder scenes keep every decision 1e-3 away, and on the random scenes NOTES.md counts the pixels below 1.5e-5);
// the bound on last_ids still trims the walk identically.  Cure, if it ever matters: sigma_log2e in k_mraster_bwd.
__device__ __forceinline__ float3 stage_conic(const float4& q1) {
  return make_float3(q1.x * (0.5f * GSL_LOG2E), q1.y * GSL_LOG2E, q1.z * (0.5f * GSL_LOG2E));
}
__device__ __forceinline__ float sigma_log2e(float ca, float cb, float cc, float dx, float dy) {
  return fmaf(cb * dx, dy, fmaf(ca * dx, dx, cc * dy * dy));
}

// ---- 7. c . v of an entry: its colour record s2[t] (D >= 3) and depth feature against the upstream gradient ----------------
template <int D>
__device__ __forceinline__ float colour_dot(const float4* s2, int t, float depth, const float (&vc)[D]) {
  float c = 0.f;
  if constexpr (D >= 3) {
    const float4 q2 = s2[t];
    c = q2.x * vc[0] + q2.y * vc[1] + q2.z * vc[2];
  }
  if constexpr (D == 1 || D == 4) c += depth * vc[D - 1];
  return c;
}

// ---- 8. the forward's write-out of a pixel: alpha, the colour sums (pix[0 .. D-1]; ED: the depth sum becomes the expected
// depth), the last composited entry
template <int D, bool ED, int N>
__device__ __forceinline__ void write_pixel(float* __restrict__ render, float* __restrict__ alphas,
                                            int32_t* __restrict__ last_ids, size_t pid, float T, float (&pix)[N], int last) {
  static_assert(D <= N, "pix holds the D channels");
  const float A = 1.f - T;
  alphas[pid] = A;
  if (ED) pix[D - 1] = pix[D - 1] / fmaxf(A, GSL_ED_ALPHA_MIN);
#pragma unroll
  for (int k = 0; k < D; ++k) render[pid * D + k] = pix[k];
  last_ids[pid] = last;
}

}  // namespace gsl
