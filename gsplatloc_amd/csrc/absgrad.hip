// Absolute screen-space gradient ("absgrad"): for every Gaussian g, sum over pixels p of |dL_p / d means2d[g]|, x and y
// separately -- gsplat's means2d.absgrad (rasterization(absgrad=True)), the densification statistic its DefaultStrategy
// reads instead of |means2d.grad| when absgrad is on.
//
// Why a kernel of its own.  The compositing backwards (raster_g16.hip, raster.hip) sum pixel moments or pixel gradients
// of a (tile, Gaussian) pair before they form v_means2d; |.| of a sum is not the sum of |.|, so every pixel's
// contribution has to be evaluated on its own.  This walk does only that: it replays the backward recurrences of every
// pixel (T /= 1 - alpha, v_alpha = T c.v - buf / (1 - alpha), buf += alpha T c.v) and forms, per (pixel, entry),
// v_xy = -opacity vis v_alpha (conic . (mean - pixel)); nothing else (no conic / opacity / colour gradient).
//
// Layout.  One 256-thread workgroup per 16x16 tile, one wave per 8x8 quadrant, one lane per pixel.  The tile's list is
// staged in LDS back to front in chunks of AB_CH entries; every wave walks the chunk's entries its quadrant composited
// (the forward's hit list when there is one, otherwise every entry up to the quadrant's last composited one); an entry
// no lane of the wave composited costs one ballot and no reduction.  A wave's sums of |v_x|, |v_y| go to an LDS slot of
// the entry (the four waves add into the same slot), and after the chunk the non-zero slots leave as 4-byte global
// atomics, two adjacent lanes per Gaussian (one 8-byte row, 32 rows per instruction).  Tile lists of any length (the pile
// of an invalid depth frame) are walked completely, chunk after chunk.
//
// Two instantiations over the record layout: FUSED reads the Q0 / Q1 / Q2 records of gsl_fused_project (channels 1 / 3 /
// 4, the depth channel's colour is Q0.z, "ED" folded into the upstream gradient as gsl_fused_raster_bwd does) and
// evaluates alpha with the operations of the fused forward (raster_px.hip); the staged one reads the SoA arrays of
// gsl_rasterize_fwd (any channel count it supports, backgrounds) with that forward's operations (raster.hip).  Both
// take the forward's alpha >= 1/255 decision for every (pixel, entry) pair -- FUSED through the functions the fused forward
// itself calls (composite_dev.h: stage_conic, sigma_log2e), which also holds the kernel's opening steps.
#include "gsloc_internal.h"
#include "composite_dev.h"

namespace gsl {

#define GSL_AB_CH 64  // list entries per staged chunk (one hit word per lane)

template <int D, bool FUSED>
struct AbStage {
  static constexpr int NC = FUSED ? 1 : GSL_AB_CH * D;
  float4 s0[GSL_AB_CH];  // FUSED: Q0 (x, y, depth, opacity); staged: (x, y, opacity, 0)
  float4 s1[GSL_AB_CH];  // conic (a, b, c, -)
  float4 s2[(FUSED && D >= 3) ? GSL_AB_CH : 1];  // FUSED: Q2 (r, g, b, 0)
  float col[NC];                                 // staged: colours [slot][D]
  int32_t id[GSL_AB_CH];
  float acc[2 * GSL_AB_CH];  // per slot: sum |v_x|, sum |v_y| over the tile's pixels
  uint8_t nzlist[GSL_AB_CH];
  int fin[4];
  int nnz;
};

template <int D, bool ED, bool FUSED>
__global__ __launch_bounds__(256) void k_absgrad(
    const float4* __restrict__ Q0, const float4* __restrict__ Q1, const float4* __restrict__ Q2,
    const float* __restrict__ means2d, const float* __restrict__ conics, const float* __restrict__ colors,
    const float* __restrict__ opacities, const float* __restrict__ backgrounds, int W, int H, int tile_w,
    const int32_t* __restrict__ tile_offsets, const int32_t* __restrict__ flatten_ids, long long capacity,
    const float* __restrict__ render, const float* __restrict__ alphas, const int32_t* __restrict__ last_ids,
    const float* __restrict__ v_render, const float* __restrict__ v_alphas, const uint32_t* __restrict__ isect_hits,
    const int32_t* __restrict__ isect_hit_counts, float* __restrict__ absgrad) {
  constexpr bool RGB = FUSED && D >= 3;
  __shared__ AbStage<D, FUSED> sb;
  const int tile = (int)blockIdx.x;
  const int tid = (int)threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const TilePixel tp = quadrant_pixel<false>(tile, tile_w, wv, lane);
  const bool inside = pixel_inside(tp, W, H, 0, H);

  ListSpan sp = tile_span(tile_offsets, tile, capacity);
  if (sp.rs >= sp.re) return;

  // per pixel: the backward's starting state
  const size_t pid = pixel_index(tp, W, inside);
  const int bin_final = last_composited(last_ids, pid, inside);
  float vc[D];
  load_upstream<D>(v_render, pid, inside, vc);
  const BwdStart st = bwd_start<D, FUSED && ED>(alphas, render, v_alphas, pid, inside, vc);
  // staged: `render` carries gsl_rasterize_fwd's t_final when the caller has it -- the pixel's last T itself, which
  // 1 - alpha no longer holds once T is small (include/gsloc_hip.h)
  float T = st.T_final;
  if (!FUSED && render && inside) T = render[pid];
  float Bp = FUSED ? st.Bp() : -T * st.va;
  if (!FUSED && backgrounds) {  // (the staged forward's background term)
    float bg_dot = 0.f;
#pragma unroll
    for (int k = 0; k < D; ++k) bg_dot += backgrounds[k] * vc[k];
    Bp += T * bg_dot;
  }

  const int qfin = wave_max(bin_final);
  if (lane == 0) sb.fin[wv] = qfin;
  // this quadrant's hit list (gsl_fused_raster_fwd): entries in list order, at 4 start + quadrant x length
  const uint32_t* qh = nullptr;
  int hp = 0;
  if (FUSED && isect_hits) {
    qh = isect_hits + 4 * sp.rs + (long long)wv * (sp.re - sp.rs);
    hp = isect_hit_counts[tile * 4 + wv];
  }
  __syncthreads();
  block_last_trim(sb.fin, sp);  // nothing behind the last entry a pixel of the tile composited

  const unsigned long long lt = (1ull << lane) - 1ull;
  for (long long hi = sp.re; hi > sp.rs; hi -= GSL_AB_CH) {
    const long long lo = max(hi - (long long)GSL_AB_CH, sp.rs);
    const int n = (int)(hi - lo);
    __syncthreads();  // (the previous chunk's flush has read id / acc)
    if (tid < n) {  // slot t <-> list index lo + t
      const int g = flatten_ids[lo + tid];
      sb.id[tid] = g;
      if (FUSED) {
        sb.s0[tid] = Q0[g];
        sb.s1[tid] = Q1[g];
        if (RGB) sb.s2[tid] = Q2[g];
      } else {
        sb.s0[tid] = make_float4(means2d[2 * (size_t)g], means2d[2 * (size_t)g + 1], opacities[g], 0.f);
        sb.s1[tid] = make_float4(conics[3 * (size_t)g], conics[3 * (size_t)g + 1], conics[3 * (size_t)g + 2], 0.f);
#pragma unroll
        for (int k = 0; k < D; ++k) sb.col[tid * D + k] = colors[(size_t)g * D + k];
      }
    }
    if (tid < 2 * GSL_AB_CH) sb.acc[tid] = 0.f;
    __syncthreads();

    // one (quadrant, entry) trip: this lane's pixel's contribution, reduced over the wave when any lane has one
    auto trip = [&](int t) {
      const float4 c0 = sb.s0[t], c1 = sb.s1[t];
      const float dx = c0.x - tp.px, dy = c0.y - tp.py;
      float sigma, vis, opv;
      if (FUSED) {  // the fused forward's
        const float3 cn = stage_conic(c1);
        sigma = sigma_log2e(cn.x, cn.y, cn.z, dx, dy);
        vis = __builtin_amdgcn_exp2f(-sigma);
        opv = c0.w * vis;
      } else {  // gsl_rasterize_fwd's
        sigma = 0.5f * (c1.x * dx * dx + c1.z * dy * dy) + c1.y * dx * dy;
        vis = __expf(-sigma);
        opv = c0.z * vis;
      }
      const float alpha = fminf(GSL_ALPHA_MAX, opv);
      const bool valid = (lo + t <= (long long)bin_final) && !(sigma < 0.f) && alpha >= GSL_ALPHA_MIN;
      if (__ballot(valid) == 0ull) return;
      float gx = 0.f, gy = 0.f;
      if (valid) {
        const float ra = 1.f / (1.f - alpha);
        T *= ra;
        const float fac = alpha * T;
        float cdot = 0.f;
        if (FUSED) {
          cdot = colour_dot<D>(sb.s2, t, c0.z, vc);
        } else {
#pragma unroll
          for (int k = 0; k < D; ++k) cdot += sb.col[t * D + k] * vc[k];
        }
        const float v_alpha = T * cdot - ra * Bp;
        Bp += fac * cdot;
        if (opv <= GSL_ALPHA_MAX) {  // (a clamped alpha has no gradient)
          const float vs = -opv * v_alpha;
          gx = vs * (c1.x * dx + c1.y * dy);
          gy = vs * (c1.y * dx + c1.z * dy);
        }
      }
      const float sx = wave_sum(fabsf(gx)), sy = wave_sum(fabsf(gy));
      if (lane == 0) {
        atomicAdd(&sb.acc[2 * t], sx);
        atomicAdd(&sb.acc[2 * t + 1], sy);
      }
    };

    if (FUSED && qh) {
      // the next (at most 64) entries of the hit list, back to front: lane k holds the k-th; those in [lo, hi) are this
      // chunk's (a hit list only holds composited entries, none at or beyond hi; anything else is consumed unused)
      const int k = hp - 1 - lane;
      long long idx = -1;
      if (k >= 0) idx = (long long)(qh[k] & GSL_HIT_INDEX_MASK);
      const unsigned long long mine = __ballot(idx >= lo);
      unsigned long long m = __ballot(idx >= lo && idx < hi);
      hp -= __popcll(mine);
      const int slot = (int)(idx - lo);
      while (m) {
        const int u = __ffsll((long long)m) - 1;
        m &= m - 1ull;
        trip(__builtin_amdgcn_readlane(slot, u));
      }
    } else {
      // every staged entry up to the last one a pixel of this quadrant composited, back to front
      unsigned long long m = __ballot(lane < n && lo + lane <= (long long)qfin);
      while (m) {
        const int t = 63 - __clzll((long long)m);
        m &= ~(1ull << t);
        trip(t);
      }
    }
    __syncthreads();

    // flush: the slots with a non-zero sum, packed; two lanes per Gaussian (x, y), 32 Gaussians per atomic instruction
    if (wv == 0) {
      const bool nz = lane < n && (sb.acc[2 * lane] != 0.f || sb.acc[2 * lane + 1] != 0.f);
      const unsigned long long mask = __ballot(nz);
      if (nz) sb.nzlist[__popcll(mask & lt)] = (uint8_t)lane;
      if (lane == 0) sb.nnz = __popcll(mask);
    }
    __syncthreads();
    if (tid < 2 * sb.nnz) {
      const int sl = sb.nzlist[tid >> 1], c = tid & 1;
      atomicAdd(&absgrad[2 * (size_t)sb.id[sl] + c], sb.acc[2 * sl + c]);
    }
  }
}

}  // namespace gsl

extern "C" int gsl_fused_absgrad(const float* Q0, const float* Q1, const float* Q2, int channels, int ed, int width,
                                 int height, int tile_w, int tile_h, const int32_t* tile_offsets,
                                 const int32_t* flatten_ids, int64_t capacity, const float* render, const float* alphas,
                                 const int32_t* last_ids, const float* v_render, const float* v_alphas,
                                 const uint32_t* isect_hits, const int32_t* isect_hit_counts, float* absgrad,
                                 void* stream) {
  if (!gsl::frame_ok(width, height, tile_w, tile_h, 0, tile_h, capacity, 0, height)) return GSL_ERR_BAD_ARG;  // (whole frame)
  if (!(channels == 1 || channels == 3 || channels == 4) || !gsl::ed_ok(channels, ed)) return GSL_ERR_BAD_ARG;
  if (!tile_offsets || !alphas || !last_ids || !v_render || !v_alphas || !absgrad) return GSL_ERR_BAD_ARG;
  if (ed && !render) return GSL_ERR_BAD_ARG;
  if ((isect_hits == nullptr) != (isect_hit_counts == nullptr)) return GSL_ERR_BAD_ARG;
  if (isect_hits && capacity >= ((int64_t)1 << GSL_HIT_SHIFT)) return GSL_ERR_BAD_ARG;
  if (capacity > 0 && (!flatten_ids || !gsl::records_ok(nullptr, Q0, Q1, Q2, channels))) return GSL_ERR_BAD_ARG;
  if (capacity == 0) return GSL_OK;
  hipStream_t st = (hipStream_t)stream;
#define CALL_AB(DD, EE)                                                                                               \
  hipLaunchKernelGGL((gsl::k_absgrad<DD, EE, true>), dim3(tile_w * tile_h), dim3(256), 0, st, (const float4*)Q0,     \
                     (const float4*)Q1, (const float4*)Q2, nullptr, nullptr, nullptr, nullptr, nullptr, width, height, \
                     tile_w, tile_offsets, flatten_ids, (long long)capacity, render, alphas, last_ids, v_render,      \
                     v_alphas, isect_hits, isect_hit_counts, absgrad)
  GSL_DISPATCH_CH_ED(channels, ed, CALL_AB)
#undef CALL_AB
  GSL_CHECK_LAUNCH();
  return GSL_OK;
}

extern "C" int gsl_rasterize_absgrad(const float* means2d, const float* conics, const float* colors,
                                     const float* opacities, const float* backgrounds, int channels, int width,
                                     int height, int tile_size, int tile_w, int tile_h, const int32_t* tile_offsets,
                                     const int32_t* flatten_ids, int64_t capacity, const float* render_alphas,
                                     const int32_t* last_ids, const float* t_final, const float* v_render_colors,
                                     const float* v_render_alphas, float* absgrad, void* stream) {
  if (!gsl::frame_ok(width, height, tile_w, tile_h, 0, tile_h, capacity, 0, height)) return GSL_ERR_BAD_ARG;  // (whole frame)
  if (tile_size != 16) return GSL_ERR_BAD_ARG;
  switch (channels) {
    case 1: case 2: case 3: case 4: case 5: case 8: case 16: case 32: break;
    default: return GSL_ERR_BAD_ARG;
  }
  if (!tile_offsets || !render_alphas || !last_ids || !v_render_colors || !v_render_alphas || !absgrad)
    return GSL_ERR_BAD_ARG;
  if (capacity > 0 && (!means2d || !conics || !colors || !opacities || !flatten_ids)) return GSL_ERR_BAD_ARG;
  if (capacity == 0) return GSL_OK;
  hipStream_t st = (hipStream_t)stream;
#define CALL_AB(DD)                                                                                                   \
  hipLaunchKernelGGL((gsl::k_absgrad<DD, false, false>), dim3(tile_w * tile_h), dim3(256), 0, st, nullptr, nullptr,  \
                     nullptr, means2d, conics, colors, opacities, backgrounds, width, height, tile_w, tile_offsets,    \
                     flatten_ids, (long long)capacity, t_final, render_alphas, last_ids, v_render_colors,             \
                     v_render_alphas, nullptr, nullptr, absgrad)
  switch (channels) {
    case 1: CALL_AB(1); break;
    case 2: CALL_AB(2); break;
    case 3: CALL_AB(3); break;
    case 4: CALL_AB(4); break;
    case 5: CALL_AB(5); break;
    case 8: CALL_AB(8); break;
    case 16: CALL_AB(16); break;
    default: CALL_AB(32); break;
  }
#undef CALL_AB
  GSL_CHECK_LAUNCH();
  return GSL_OK;
}
