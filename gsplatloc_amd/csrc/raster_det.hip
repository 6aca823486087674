// Deterministic compositing backward of the fused pipeline (k_mraster_bwd; gsl_fused_raster_bwd with vrow given).  The
// default, non-deterministic backward is raster_g16.hip.  256-thread workgroup per 16x16 tile, one wave64 per 8x8
// quadrant; a batch of list entries is gathered once per workgroup into LDS, each wave ballots the quadrant test over 64
// of them and walks the survivors back to front, broadcasting each record from LDS (wave-uniform address).  The
// per-splat pixel sums run on the matrix cores (the 64-lane DPP reduce-scatter of 7-10 values per splat they replaced cost a
// quarter of the kernel: profiles/r02_backward_ablation.txt).  Every one of those sums is linear in two per-pixel
// scalars of the (pixel, splat) pair,
//     w = vis * v_alpha (0 where alpha is clamped or the pixel did not composite the splat)    f = alpha * T,
// with per-pixel weights that do not depend on the splat once dx = X - px is expanded around the tile centre:
//     sum_p w * {1, lx, ly, lx^2, lx ly, ly^2}      (lx, ly = pixel centre - tile centre)
//     sum_p f * v_colour_k(p)
// i.e. [splats x pixels] . [pixels x 16] products.  The walk stores w and f of 8 splats as rows of a 16 x 64 tile in
// LDS (lane = pixel = column: conflict-free stores); 16 v_mfma_f32_16x16x4_f32 (exact f32 fma chains) then produce the
// 8 x (6 + CG) sums.  A wave meets a batch slot at most once per batch, so the sums are plain stores into the wave's OWN
// copy of the slot's moment row.  At the end of a batch one thread per slot adds the four copies in wave order, turns the
// moments into the gradient row  [v_xy | v_conic | v_opacity | v_colour]  (X, Y, conic and opacity are the splat's
// own) and stores it in the row of its INTERSECTION, vrow[capacity][16] (zero rows included; rows of entries that are
// not walked are zeroed up front).  No atomic anywhere: the projection backward (fused_project_bwd.hip) finds a Gaussian's
// rows by binary search in the sorted tile lists and adds them in tile order.  The matrix pipe runs beside the vector
// pipe, so the reduction costs the walk ~2 LDS stores per splat.  The kernel's opening (list span, lane -> pixel, starting
// state, trim to the tile's last composited entry) is composite_dev.h's; alpha here is the __expf form.
#include "gsloc_internal.h"
#include "composite_dev.h"

namespace gsl {

typedef float gsl_f32x4 __attribute__((ext_vector_type(4)));

#define GSL_MB 192        // list entries staged per batch (three 64-entry chunks)
#define GSL_MPITCH 72     // floats per tile row: 16-byte reads of lane (k, i) at [i][16 m + 4 k] hit 16 distinct bank quads

template <int D>
struct FStageM {
  static constexpr int A = 6 + D;   // moment / gradient row: [6 geometric][D colour]
  static constexpr int AP = A | 1;  // odd LDS pitch
  static constexpr int NW = 4;      // one moment row per (wave, slot), summed in wave order
  float4 s0[GSL_MB];
  float4 s1[GSL_MB];
  float4 s2[(D >= 3) ? GSL_MB : 1];
  float acc[NW * GSL_MB * AP];        // per-(wave, slot) moments
  float tile[4][16 * GSL_MPITCH];     // per wave: rows 0-7 = w of the group's splats, rows 8-15 = f
  int32_t gslot[4][8];                // batch slot of each splat of the group
};

template <int D, int CG>
__device__ __forceinline__ void mraster_group_flush(FStageM<D>& sb, int wv, int lane, int count,
                                                    const float (&bmat)[16]) {
  // D[i][j] = sum_k A[i][k] B[k][j]; lane l holds A[i = l & 15][k = l >> 4] and B[k = l >> 4][j = l & 15]; K-step kb
  // of lane-row k is pixel 16 (kb >> 2) + 4 k + (kb & 3); result row 4 (l >> 4) + r, column l & 15 in register r.
  constexpr int AP = FStageM<D>::AP;
  int k = lane >> 4, ij = lane & 15;
  const float* row = &sb.tile[wv][ij * GSL_MPITCH + 4 * k];
  gsl_f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
  // rows 0-7 (w) meet the monomial columns, rows 8-15 (f) the colour columns: one B per lane serves both because
  // the unwanted blocks of the product are simply not read back
#pragma unroll
  for (int m = 0; m < 4; ++m) {
    float4 a = *reinterpret_cast<const float4*>(row + 16 * m);
    float av[4] = {a.x, a.y, a.z, a.w};
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      int kb = 4 * m + u;
      if (u & 1) acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(av[u], bmat[kb], acc1, 0, 0, 0);
      else acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(av[u], bmat[kb], acc0, 0, 0, 0);
    }
  }
  float d[4] = {acc0[0] + acc1[0], acc0[1] + acc1[1], acc0[2] + acc1[2], acc0[3] + acc1[3]};
  // lane rows 0,1 hold the w rows (splat 4 k + r), columns < 6; lane rows 2,3 the f rows (splat 4 (k - 2) + r),
  // columns 6 .. 6 + CG - 1
  bool wrow = k < 2;
  int sbase = 4 * (k & 1);
  bool col_ok = wrow ? (ij < 6) : (ij >= 6 && ij < 6 + CG);
  int col = (CG == D || wrow) ? ij : (6 + D - 1);  // depth-only variant: its single colour column is the last one
  int4 gs = *reinterpret_cast<const int4*>(&sb.gslot[wv][sbase]);
  int sl[4] = {gs.x, gs.y, gs.z, gs.w};
#pragma unroll
  for (int r = 0; r < 4; ++r)
    if (col_ok && sbase + r < count && d[r] != 0.f) {
      // a wave visits a slot once per batch: a plain store into the wave's own copy of the row
      sb.acc[(wv * GSL_MB + sl[r]) * AP + col] = d[r];
    }
}

template <int D, int CG>
__device__ __forceinline__ void mraster_bwd_body(
    FStageM<D>& sb, const float4* __restrict__ Q0, const float4* __restrict__ Q1, const float4* __restrict__ Q2,
    const uint4* __restrict__ Qh, const int32_t* __restrict__ flatten_ids, float* __restrict__ vacc, long long rs,
    long long re, int nb, int tid, float px, float py, float qcx, float qcy, float tcx, float tcy, bool inside,
    int bin_final, int wave_final, float T_final, const float (&vc)[D], float va) {
  constexpr bool RGB = D >= 3;
  constexpr int A = FStageM<D>::A;
  constexpr int AP = FStageM<D>::AP;
  constexpr int NW = FStageM<D>::NW;
  int lane = tid & 63, wv = tid >> 6;
  float T = T_final;
  float Bp = -T_final * va;
  unsigned long long insidem = __ballot(inside);
  // B operand of this lane: K-step kb of lane-row k is pixel (= walk lane) pl = 16 (kb >> 2) + 4 k + (kb & 3)
  float phi[16], bcol[16];
  {
    int k = lane >> 4, j = lane & 15;
    float wlx = __shfl(px - tcx, 0, 64), wly = __shfl(py - tcy, 0, 64);  // offset of the quadrant's first pixel
#pragma unroll
    for (int kb = 0; kb < 16; ++kb) {
      int pl = 16 * (kb >> 2) + 4 * k + (kb & 3);
      float lx = wlx + (float)(pl & 7), ly = wly + (float)(pl >> 3);
      float m = (j == 0) ? 1.f : (j == 1) ? lx : (j == 2) ? ly : (j == 3) ? lx * lx : (j == 4) ? lx * ly : (j == 5) ? ly * ly : 0.f;
      phi[kb] = m;
      bcol[kb] = 0.f;
    }
  }
  if (CG == D) {
    // colour columns: B[pixel][6 + ch] = upstream gradient of channel ch at that pixel
    // (exchanged once through this wave's tile, which is not in use yet)
    float* vcs = sb.tile[wv];
#pragma unroll
    for (int ch = 0; ch < D; ++ch) vcs[lane * D + ch] = vc[ch];
    wave_lds_fence();
    int k = lane >> 4, j = lane & 15;
#pragma unroll
    for (int kb = 0; kb < 16; ++kb) {
      int pl = 16 * (kb >> 2) + 4 * k + (kb & 3);
      if (j >= 6 && j < 6 + D) bcol[kb] = vcs[pl * D + (j - 6)];
    }
    wave_lds_fence();
  } else {
    int j = lane & 15;
#pragma unroll
    for (int kb = 0; kb < 16; ++kb) bcol[kb] = (j == 6) ? 1.f : 0.f;  // f already carries v_depth of its pixel
  }
  float bmat[16];  // this lane's column of B: a monomial column (j < 6) or a colour column
#pragma unroll
  for (int kb = 0; kb < 16; ++kb) bmat[kb] = ((lane & 15) < 6) ? phi[kb] : bcol[kb];
  float* wrow = &sb.tile[wv][lane];

  // The records of batch b + 1 are gathered into registers while batch b is walked (the gather is two dependent
  // global loads per thread; nothing else in the kernel can cover their latency at 3 workgroups per CU).
  int pg = 0;
  float4 pr0 = make_float4(0.f, 0.f, 0.f, 0.f), pr1 = pr0, pr2 = pr0;
  auto gather = [&](int b) {
    long long bend = re - 1 - (long long)b * GSL_MB;
    int bsize = (int)min((long long)GSL_MB, bend + 1 - rs);
    if (tid < bsize) {
      pg = flatten_ids[bend - tid];
      load_record(Q0, Q1, Q2, Qh, pg, RGB && CG == D, pr0, pr1, pr2);
    }
  };
  gather(0);

  for (int b = 0; b < nb; ++b) {
    long long bend = re - 1 - (long long)b * GSL_MB;  // slot t <-> absolute index bend - t (back to front)
    int bsize = (int)min((long long)GSL_MB, bend + 1 - rs);
    __syncthreads();
    if (tid < bsize) {
      sb.s0[tid] = pr0;
      sb.s1[tid] = pr1;
      if (RGB && CG == D) sb.s2[tid] = pr2;
    }
    if (tid < GSL_MB) {
#pragma unroll
      for (int w = 0; w < NW; ++w)
#pragma unroll
        for (int k = 0; k < A; ++k) sb.acc[(w * GSL_MB + tid) * AP + k] = 0.f;
    }
    __syncthreads();
    if (b + 1 < nb) gather(b + 1);
    int t_first = (int)max((long long)0, bend - (long long)wave_final);
    int hh = 0;  // splats in the open group
    for (int c = (t_first / 64) * 64; c < bsize; c += 64) {
      int e = c + lane;
      float4 a0 = make_float4(0.f, 0.f, 0.f, 0.f), a1 = make_float4(0.f, 0.f, 0.f, -1.f);
      if (e < bsize && e >= t_first) {
        a0 = sb.s0[e];
        a1 = sb.s1[e];
      }
      unsigned long long m = __ballot(fabsf(a0.x - qcx) <= a1.w + 3.5f) & __ballot(fabsf(a0.y - qcy) <= a1.w + 3.5f);
      if (!m) continue;
      int t = c + __ffsll((long long)m) - 1;
      m &= m - 1;
      float4 q0 = sb.s0[t], q1 = sb.s1[t];
      for (;;) {
        // the next survivor's records are requested before this one's arithmetic (wave-uniform LDS addresses)
        bool more = m != 0;
        int tn = t;
        float4 q0n = q0, q1n = q1;
        if (more) {
          tn = c + __ffsll((long long)m) - 1;
          m &= m - 1;
          q0n = sb.s0[tn];
          q1n = sb.s1[tn];
        }
        float dx = q0.x - px, dy = q0.y - py;
        float gx = q1.x * dx + q1.y * dy;
        float gy = q1.y * dx + q1.z * dy;
        float sigma = 0.5f * (dx * gx + dy * gy);
        float vis = __expf(-sigma);
        float opv = q0.w * vis;
        float alpha = fminf(GSL_ALPHA_MAX, opv);
        unsigned long long validm = insidem & __ballot((int)(bend - t) <= bin_final) & __ballot(sigma >= 0.f) &
                                    __ballot(alpha >= GSL_ALPHA_MIN);
        if (validm) {  // some pixel of this quadrant composited the splat
          unsigned long long capm = __ballot(opv <= GSL_ALPHA_MAX);
          float am = sel(validm, alpha, 0.f);  // other lanes: alpha = 0 => ra = 1, fac = 0, nothing changes
          float ra = __builtin_amdgcn_rcpf(1.f - am);
          T *= ra;
          float fac = am * T;
          const float cdot = (CG == D) ? colour_dot<D>(sb.s2, t, q0.z, vc) : q0.z * vc[D - 1];
          float v_alpha = T * cdot - ra * Bp;
          Bp += fac * cdot;
          float vism = sel(validm & capm, vis, 0.f);  // alpha clamped at 0.999 => no geometric gradient
          wrow[hh * GSL_MPITCH] = vism * v_alpha;
          wrow[(8 + hh) * GSL_MPITCH] = (CG == D) ? fac : fac * vc[D - 1];
          if (lane == 0) sb.gslot[wv][hh] = t;
          if (++hh == 8) {
            wave_lds_fence();
            mraster_group_flush<D, CG>(sb, wv, lane, 8, bmat);
            wave_lds_fence();
            hh = 0;
          }
        }
        if (!more) break;
        t = tn;
        q0 = q0n;
        q1 = q1n;
      }
    }
    if (hh) {
      wave_lds_fence();
      mraster_group_flush<D, CG>(sb, wv, lane, hh, bmat);
      wave_lds_fence();
    }
    __syncthreads();
    // Moments -> gradient row (one thread per slot).
    {
      bool nz = false;
      float mo[A];
#pragma unroll
      for (int k = 0; k < A; ++k) mo[k] = 0.f;
      if (tid < bsize) {
#pragma unroll
        for (int k = 0; k < A; ++k) {
          float m = sb.acc[tid * AP + k];
#pragma unroll
          for (int w = 1; w < NW; ++w) m += sb.acc[(w * GSL_MB + tid) * AP + k];  // fixed wave order
          mo[k] = m;
          nz = nz || (m != 0.f);
        }
        if (nz) {
          float4 q0 = sb.s0[tid], q1 = sb.s1[tid];
          float X = q0.x - tcx, Y = q0.y - tcy, S = mo[0];
          float Sx = X * S - mo[1], Sy = Y * S - mo[2];
          float Sxx = X * (X * S - 2.f * mo[1]) + mo[3];
          float Sxy = X * (Y * S - mo[2]) - Y * mo[1] + mo[4];
          float Syy = Y * (Y * S - 2.f * mo[2]) + mo[5];
          float no = -q0.w;  // v_sigma = -opacity * w
          mo[0] = no * (q1.x * Sx + q1.y * Sy);
          mo[1] = no * (q1.y * Sx + q1.z * Sy);
          mo[2] = 0.5f * no * Sxx;
          mo[3] = no * Sxy;
          mo[4] = 0.5f * no * Syy;
          mo[5] = S;
        }
      }
      // the (tile, splat) row goes to the intersection's own slot with plain stores (zero rows included); the
      // projection backward sums a Gaussian's rows in tile order
      if (tid < bsize) {
        float pad[12];
#pragma unroll
        for (int k = 0; k < 12; ++k) pad[k] = (k < A && nz) ? mo[k] : 0.f;
        float4* dst = reinterpret_cast<float4*>(vacc) + 4 * (size_t)(bend - tid);
        dst[0] = make_float4(pad[0], pad[1], pad[2], pad[3]);
        dst[1] = make_float4(pad[4], pad[5], pad[6], pad[7]);
        dst[2] = make_float4(pad[8], pad[9], pad[10], pad[11]);
      }
    }
  }
}

template <int D, bool ED>
__global__ __launch_bounds__(256) void k_mraster_bwd(
    const float4* __restrict__ Q0, const float4* __restrict__ Q1, const float4* __restrict__ Q2, int W, int H,
    int tile_w, int ty0, const int32_t* __restrict__ tile_offsets, const int32_t* __restrict__ flatten_ids,
    long long capacity, const float* __restrict__ render, const float* __restrict__ alphas,
    const int32_t* __restrict__ last_ids, const float* __restrict__ v_render, const float* __restrict__ v_alphas,
    float* __restrict__ vacc, int row0, int row1, const uint4* __restrict__ Qh) {
  // vacc is vrow[capacity][16], one row per intersection
  __shared__ FStageM<D> sb;
  __shared__ int s_final[4];
  int tile = ty0 * tile_w + GSL_TILE_OF_BLOCK();
  int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const TilePixel tp = quadrant_pixel<false>(tile, tile_w, wv, lane);
  bool inside = pixel_inside(tp, W, H, row0, row1);
  float qcx = (float)tp.qx + 4.f, qcy = (float)tp.qy + 4.f;
  float tcx = (float)(tp.txi * 16) + 8.f, tcy = (float)(tp.tyi * 16) + 8.f;

  ListSpan sp = tile_span(tile_offsets, tile, capacity);
  if (sp.rs >= sp.re) return;

  size_t pid = pixel_index(tp, W, inside);
  int bin_final = last_composited(last_ids, pid, inside);
  float vc[D];
  load_upstream<D>(v_render, pid, inside, vc);
  const BwdStart st = bwd_start<D, ED>(alphas, render, v_alphas, pid, inside, vc);
  int wave_final = wave_max(bin_final);
  if (lane == 0) s_final[wv] = wave_final;
  bool rgb_grad = false;
  if (D == 4) rgb_grad = (vc[0] != 0.f) || (vc[1] != 0.f) || (vc[2] != 0.f);
  int any_rgb = __syncthreads_or(rgb_grad);  // (also the barrier in front of block_last_trim)
  // nothing behind the tile's last composited entry is walked
  const long long re_all = sp.re;
  block_last_trim(s_final, sp);
  const long long rs = sp.rs, re = sp.re;
  {  // rows of the entries that are not walked are zero
    float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
    for (long long q = 4 * re + tid; q < 4 * re_all; q += 256) reinterpret_cast<float4*>(vacc)[q] = z;
  }
  if (rs >= re) return;
  int nb = (int)((re - rs + GSL_MB - 1) / GSL_MB);
  if (D == 4 && !any_rgb)
    mraster_bwd_body<D, 1>(sb, Q0, Q1, Q2, Qh, flatten_ids, vacc, rs, re, nb, tid, tp.px, tp.py, qcx, qcy, tcx, tcy, inside,
                           bin_final, wave_final, st.T_final, vc, st.va);
  else
    mraster_bwd_body<D, D>(sb, Q0, Q1, Q2, Qh, flatten_ids, vacc, rs, re, nb, tid, tp.px, tp.py, qcx, qcy, tcx, tcy, inside,
                           bin_final, wave_final, st.T_final, vc, st.va);
}

int launch_mraster_bwd(const float* Q0, const float* Q1, const float* Q2, int channels, int ed, int width, int height,
                       int tile_w, int ty0, int ty1, const int32_t* tile_offsets, const int32_t* flatten_ids,
                       int64_t capacity, const float* render, const float* alphas, const int32_t* last_ids,
                       const float* v_render, const float* v_alphas, float* vrow, int row0, int row1, const void* Qh,
                       hipStream_t st) {
  int nblk = (ty1 - ty0) * tile_w;
#define CALL_MD(DD, EE)                                                                                             \
  hipLaunchKernelGGL((k_mraster_bwd<DD, EE>), dim3(nblk), dim3(256), 0, st, (const float4*)Q0, (const float4*)Q1,   \
                     (const float4*)Q2, width, height, tile_w, ty0, tile_offsets, flatten_ids, (long long)capacity, \
                     render, alphas, last_ids, v_render, v_alphas, vrow, row0, row1, (const uint4*)Qh)
  GSL_DISPATCH_CH_ED(channels, ed, CALL_MD)
#undef CALL_MD
  GSL_CHECK_LAUNCH();
  return GSL_OK;
}

}  // namespace gsl
