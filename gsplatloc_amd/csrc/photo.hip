// Photometric term of the tracker's loss on the device: masked RGB L1 + SSIM, value and gradient with respect to the
// three colour channels of the render.  The reference declares the term and keeps it commented out
// (gs_trainer_total.py:111-123; ssim_lambda = 0.5 at data/base.py:26, StructuralSimilarityIndexMeasure(data_range=1.0)):
//
//   m     = (render[...,3] != 0)  (no gradient),   c = render[...,:3] * m,   p = pixels * m
//   l1    = sum |c - p| / (sum m + 1e-8)                                  (sum m counts pixels, not channel values)
//   ssim  = mean over the 3 (H-10) (W-10) windows that lie inside the image of
//           S = (2 mx my + C1)(2 sxy + C2) / ((mx^2 + my^2 + C1)(sx + sy + C2)),   C1 = 1e-4, C2 = 9e-4,
//           mx = w*c, my = w*p, sx = max(w*c^2 - mx^2, 0), sy likewise, sxy = w*(c p) - mx my,
//           w = g (x) g, g = 11 taps of a sigma = 1.5 Gaussian normalised to sum 1 (torchmetrics' default window)
//   photo = (1 - ssim_lambda) l1 + ssim_lambda (1 - ssim);   the kernels deliver rgb_lambda * photo.
//
// Two launches, 16x16 pixel blocks of 256 threads, the window applied separably (rows, then columns) on a 26x26 tile in
// LDS.  k_photo_stats: per block the partial sums (sum m, sum |c - p|, sum S) and, per window position and channel,
// the three derivatives the gradient needs.  k_photo_grad: every block sums the count partials in one fixed order (the
// L1 gradient's scale), gathers the three derivative maps through the same window and writes v_render[...,0:3].
// No atomics, no scratch, no allocation; every sum has a fixed order.
#include "gsloc_internal.h"

namespace gsl {

constexpr int PH_WIN = 11;                 // taps of the window per axis
constexpr int PH_TILE = 16 + PH_WIN - 1;   // side of a block's tile with its apron: 26
// Row stride of the float tiles.  ds_read_b32 banks are (address / 4) % 32 and conflicts count within a 32-lane half,
// which in the row pass is two tile rows of 16 columns: a stride of 16 (mod 32) puts them on disjoint banks for every tap.
constexpr int PH_STRIDE = 48;
constexpr double PH_C1 = 1e-4, PH_C2 = 9e-4;
// exp(-((k - 5) / 1.5)^2 / 2) / their sum, k = 0..10
#define GSL_PHOTO_TAPS                                                                                         \
  {0.0010283800844791092, 0.007598758135239185, 0.03600077212843083, 0.10936068950970002, 0.2130055377112537, \
   0.26601172486179436,   0.2130055377112537,   0.10936068950970002, 0.03600077212843083, 0.007598758135239185, \
   0.0010283800844791092}

// sum_k g[k] s[k * STEP] in the accumulator's type; g in double, rounded to A once per tap at compile time
template <typename A, int STEP, typename T>
__device__ __forceinline__ A window_sum(const T* s) {
  constexpr double g[PH_WIN] = GSL_PHOTO_TAPS;
  A a = (A)0;
#pragma unroll
  for (int k = 0; k < PH_WIN; ++k) a += (A)g[k] * (A)s[k * STEP];
  return a;
}

struct PhotoStatsLds {
  float c[PH_TILE][PH_STRIDE], p[PH_TILE][PH_STRIDE];  // one channel of the masked images at (y0 + yy, x0 + xx)
  double h[5][PH_TILE][16];  // row pass of (c, p, c c, p p, c p) of that channel
  float red[4][3];
};

// Block (x0, y0): its 256 pixels' share of (sum m, sum |c - p|) and the windows whose top-left pixel they are.  The five
// window moments are accumulated in double: sx = w*c^2 - mx^2 loses 1e-7 of c^2 in float32, which against C2 = 9e-4 is
// 1e-4 of S where the images are flat (products of two floats are exact in double, so what is left is the weights').
// maps[ch][3][nW] (nW = (H-10)(W-10) window positions, row-major): G = dS/dmx - 2 (mx - 1/2) dS/dsx - (my - 1/2) dS/dsxy,
// dS/dsx (0 where the clamp is active) and dS/dsxy, so that
//   d sum S / d c(q) = sum_p w(p - q) [G(p) + 2 (c(q) - 1/2) dS/dsx(p) + (p(q) - 1/2) dS/dsxy(p)]
// (the 1/2 cancels exactly; it keeps the float32 terms of the gather small).
// One channel at a time goes through LDS (27 KB: five blocks per CU, a 640x480 frame's 1200 blocks in one round), the
// next channel's tile being fetched into registers while this channel's two passes run.
__global__ __launch_bounds__(256) void k_photo_stats(const float* __restrict__ render, const float* __restrict__ pixels,
                                                     int W, int H, float* __restrict__ partial,
                                                     float* __restrict__ maps) {
  __shared__ PhotoStatsLds L;
  const int tid = threadIdx.x, ly = tid >> 4, lx = tid & 15;
  const int x0 = blockIdx.x * 16, y0 = blockIdx.y * 16;
  const int Wv = W - (PH_WIN - 1), Hv = H - (PH_WIN - 1);
  const size_t nW = (size_t)Wv * Hv;
  float cnt = 0.f, l1 = 0.f, sS = 0.f;
  // Tile element e = tid + 256 n of (tile row, tile column), n < PH_FETCH.  Every load leaves at once from an address
  // clamped into the image; mask and image border select afterwards (a branch on the depth would put the colour loads
  // behind a second trip to memory).
  constexpr int PH_FETCH = (PH_TILE * PH_TILE + 255) / 256;
  float nc[PH_FETCH], np[PH_FETCH];
  auto fetch = [&](int ch) {
#pragma unroll
    for (int n = 0; n < PH_FETCH; ++n) {
      int e = tid + 256 * n;
      int yy = e / PH_TILE, xx = e - yy * PH_TILE;
      int y = y0 + yy, x = x0 + xx;
      size_t q = (size_t)min(y, H - 1) * W + min(x, W - 1);
      float cv = render[q * 4 + ch], pv = pixels[q * 3 + ch];
      const bool vis = y < H && x < W && render[q * 4 + 3] != 0.f;
      nc[n] = vis ? cv : 0.f;
      np[n] = vis ? pv : 0.f;
      if (vis && yy < 16 && xx < 16) {  // (yy < 16 also keeps e inside the tile)
        if (ch == 0) cnt += 1.f;
        l1 += fabsf(cv - pv);
      }
    }
  };
  fetch(0);
  const bool has_window = y0 + ly < Hv && x0 + lx < Wv;
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) {
#pragma unroll
    for (int n = 0; n < PH_FETCH; ++n) {
      int e = tid + 256 * n;
      int yy = e / PH_TILE, xx = e - yy * PH_TILE;
      if (e < PH_TILE * PH_TILE) { L.c[yy][xx] = nc[n]; L.p[yy][xx] = np[n]; }
    }
    __syncthreads();
    if (ch < 2) fetch(ch + 1);
    for (int e = tid; e < PH_TILE * 16; e += 256) {
      int r = e >> 4, x = e & 15;
      const float* cr = &L.c[r][x];
      const float* pr = &L.p[r][x];
      constexpr double g[PH_WIN] = GSL_PHOTO_TAPS;
      double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0, a4 = 0.0;
#pragma unroll
      for (int k = 0; k < PH_WIN; ++k) {
        double cd = cr[k], pd = pr[k], gc = g[k] * cd, gp = g[k] * pd;
        a0 += gc; a1 += gp; a2 += gc * cd; a3 += gp * pd; a4 += gc * pd;
      }
      L.h[0][r][x] = a0; L.h[1][r][x] = a1; L.h[2][r][x] = a2; L.h[3][r][x] = a3; L.h[4][r][x] = a4;
    }
    __syncthreads();
    if (has_window) {
      double mx = window_sum<double, 16>(&L.h[0][ly][lx]), my = window_sum<double, 16>(&L.h[1][ly][lx]);
      double vx = window_sum<double, 16>(&L.h[2][ly][lx]) - mx * mx;
      double vy = window_sum<double, 16>(&L.h[3][ly][lx]) - my * my;
      double sxy = window_sum<double, 16>(&L.h[4][ly][lx]) - mx * my;
      double sx = fmax(vx, 0.0), sy = fmax(vy, 0.0);
      double A1 = 2.0 * mx * my + PH_C1, A2 = 2.0 * sxy + PH_C2;
      double B1 = mx * mx + my * my + PH_C1, B2 = sx + sy + PH_C2;
      double inv = 1.0 / (B1 * B2);
      double S = A1 * A2 * inv;
      double dmx = 2.0 * my * A2 * inv - 2.0 * mx * S / B1;
      double dsx = vx < 0.0 ? 0.0 : -S / B2;  // torch.clamp passes the gradient on at the bound itself
      double dsxy = 2.0 * A1 * inv;
      sS += (float)S;
      size_t wq = (size_t)(y0 + ly) * Wv + (x0 + lx);
      float* o = maps + (size_t)ch * 3 * nW + wq;
      o[0] = (float)(dmx - 2.0 * (mx - 0.5) * dsx - (my - 0.5) * dsxy);
      o[nW] = (float)dsx;
      o[2 * nW] = (float)dsxy;
    }
    // (no barrier here: the next channel's stores to c / p follow the barrier behind the row pass that read them, and
    // its row pass, which overwrites h, follows the barrier behind those stores)
  }
  int lane = tid & 63, wv = tid >> 6;
  float s0 = wave_sum(cnt), s1 = wave_sum(l1), s2 = wave_sum(sS);
  if (lane == 0) { L.red[wv][0] = s0; L.red[wv][1] = s1; L.red[wv][2] = s2; }
  __syncthreads();
  if (tid < 3)
    partial[3 * ((size_t)blockIdx.y * gridDim.x + blockIdx.x) + tid] =
        L.red[0][tid] + L.red[1][tid] + L.red[2][tid] + L.red[3][tid];
}

struct PhotoGradLds {
  float m[3][PH_TILE][PH_STRIDE];  // the three maps of one channel at window (y0 - 10 + yy, x0 - 10 + xx); 0 where none
  float h[3][PH_TILE][16];         // their row pass
  float red[4][3];
};

// Block (x0, y0): v_render[...,0:3] of its 256 pixels.  k_ssim = -rgb_lambda ssim_lambda / (3 nW), k_l1 = rgb_lambda
// (1 - ssim_lambda); the L1 scale 1 / (sum m + 1e-8) needs the whole frame's count, which every block sums from the nb
// block partials in the same fixed order.  Block (0, 0) also leaves the three sums in photo_sums.
__global__ __launch_bounds__(256) void k_photo_grad(const float* __restrict__ render, const float* __restrict__ pixels,
                                                    int W, int H, const float* __restrict__ partial, int nb,
                                                    const float* __restrict__ maps, float k_ssim, float k_l1,
                                                    float* __restrict__ v_render, float* __restrict__ photo_sums) {
  __shared__ PhotoGradLds L;
  const int tid = threadIdx.x, ly = tid >> 4, lx = tid & 15;
  const int x0 = blockIdx.x * 16, y0 = blockIdx.y * 16;
  const int Wv = W - (PH_WIN - 1), Hv = H - (PH_WIN - 1);
  const size_t nW = (size_t)Wv * Hv;
  const bool first = blockIdx.x == 0 && blockIdx.y == 0;
  // The 3 x 26 x 26 map values of a channel: element e = tid + 256 n of (map, tile row, tile column), n < PH_FETCH.  They
  // are fetched into registers one channel ahead -- the first beside the count partials below, the others while the
  // previous channel's two passes run -- so that no pass waits for memory.
  constexpr int PH_FETCH = (3 * PH_TILE * PH_TILE + 255) / 256;
  float nxt[PH_FETCH];
  auto fetch = [&](int ch) {
    const float* mc = maps + (size_t)ch * 3 * nW;
#pragma unroll
    for (int n = 0; n < PH_FETCH; ++n) {
      int e = tid + 256 * n;
      int t = e / (PH_TILE * PH_TILE), r = e - t * (PH_TILE * PH_TILE);
      int yy = r / PH_TILE, xx = r - yy * PH_TILE;
      int wy = y0 - (PH_WIN - 1) + yy, wx = x0 - (PH_WIN - 1) + xx;
      bool in = e < 3 * PH_TILE * PH_TILE && wy >= 0 && wy < Hv && wx >= 0 && wx < Wv;
      nxt[n] = in ? mc[(size_t)t * nW + (size_t)wy * Wv + wx] : 0.f;
    }
  };
  fetch(0);
  {
    float a0 = 0.f, a1 = 0.f, a2 = 0.f;
    for (int b = tid; b < nb; b += 256) {
      a0 += partial[3 * (size_t)b];
      if (first) { a1 += partial[3 * (size_t)b + 1]; a2 += partial[3 * (size_t)b + 2]; }
    }
    int lane = tid & 63, wv = tid >> 6;
    float s0 = wave_sum(a0), s1 = wave_sum(a1), s2 = wave_sum(a2);
    if (lane == 0) { L.red[wv][0] = s0; L.red[wv][1] = s1; L.red[wv][2] = s2; }
  }
  const int i = y0 + ly, j = x0 + lx;
  const bool has_pixel = i < H && j < W;
  const size_t q = (size_t)min(i, H - 1) * W + min(j, W - 1);  // (clamped: the loads leave before the mask is known)
  float cv[3], pv[3];
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) { cv[ch] = render[q * 4 + ch]; pv[ch] = pixels[q * 3 + ch]; }
  const bool vis = has_pixel && render[q * 4 + 3] != 0.f;
  __syncthreads();
  const float count = L.red[0][0] + L.red[1][0] + L.red[2][0] + L.red[3][0];
  if (first && tid < 3) photo_sums[tid] = L.red[0][tid] + L.red[1][tid] + L.red[2][tid] + L.red[3][tid];
  const float l1_scale = k_l1 / (count + 1e-8f);
  float out[3];
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) {
#pragma unroll
    for (int n = 0; n < PH_FETCH; ++n) {
      int e = tid + 256 * n;
      int t = e / (PH_TILE * PH_TILE), r = e - t * (PH_TILE * PH_TILE);
      int yy = r / PH_TILE, xx = r - yy * PH_TILE;
      if (e < 3 * PH_TILE * PH_TILE) L.m[t][yy][xx] = nxt[n];
    }
    __syncthreads();
    if (ch < 2) fetch(ch + 1);
    for (int e = tid; e < 3 * PH_TILE * 16; e += 256) {
      int t = e / (PH_TILE * 16), r = (e - t * (PH_TILE * 16)) >> 4, x = e & 15;
      L.h[t][r][x] = window_sum<float, 1>(&L.m[t][r][x]);
    }
    __syncthreads();
    // pixel (ly, lx) is tap (10 - k, 10 - k') of the window at tile position (ly + k, lx + k'); the window is symmetric
    float g = window_sum<float, 16>(&L.h[0][ly][lx]) + 2.f * (cv[ch] - 0.5f) * window_sum<float, 16>(&L.h[1][ly][lx]) +
              (pv[ch] - 0.5f) * window_sum<float, 16>(&L.h[2][ly][lx]);
    float d = cv[ch] - pv[ch];
    float sgn = d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f);
    out[ch] = vis ? k_ssim * g + l1_scale * sgn : 0.f;
    // (no barrier here: the next channel's stores to m follow the barrier behind the row pass that read it, and its row
    // pass, which overwrites h, follows the barrier behind those stores)
  }
  if (has_pixel) {
    v_render[q * 4 + 0] = out[0];
    v_render[q * 4 + 1] = out[1];
    v_render[q * 4 + 2] = out[2];
  }
}

static inline int photo_blocks(int width, int height) { return ((width + 15) / 16) * ((height + 15) / 16); }
// partials [nb][3], padded to 16 bytes
static inline size_t photo_maps_offset(int width, int height) {
  return (((size_t)photo_blocks(width, height) * 3 * sizeof(float)) + 15) & ~(size_t)15;
}

}  // namespace gsl

extern "C" size_t gsl_photo_ws_bytes(int width, int height) {
  if (width < gsl::PH_WIN || height < gsl::PH_WIN) return 0;
  size_t nW = (size_t)(width - (gsl::PH_WIN - 1)) * (size_t)(height - (gsl::PH_WIN - 1));
  return gsl::photo_maps_offset(width, height) + 9 * nW * sizeof(float);
}

extern "C" int gsl_photo_loss(const float* render, int channels, const float* pixels, int width, int height,
                              float rgb_lambda, float ssim_lambda, float* v_render, float* photo_sums, void* ws,
                              size_t ws_bytes, void* stream) {
  if (!render || !pixels || !v_render || !photo_sums || !ws || channels != 4) return GSL_ERR_BAD_ARG;
  if (width < gsl::PH_WIN || height < gsl::PH_WIN) return GSL_ERR_BAD_ARG;
  if (ws_bytes < gsl_photo_ws_bytes(width, height)) return GSL_ERR_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  float* partial = (float*)ws;
  float* maps = (float*)((char*)ws + gsl::photo_maps_offset(width, height));
  dim3 grid((width + 15) / 16, (height + 15) / 16);
  int nb = gsl::photo_blocks(width, height);
  double nS = 3.0 * (double)(width - (gsl::PH_WIN - 1)) * (double)(height - (gsl::PH_WIN - 1));
  hipLaunchKernelGGL(gsl::k_photo_stats, grid, dim3(256), 0, st, render, pixels, width, height, partial, maps);
  GSL_CHECK_LAUNCH();
  hipLaunchKernelGGL(gsl::k_photo_grad, grid, dim3(256), 0, st, render, pixels, width, height, partial, nb, maps,
                     (float)(-(double)rgb_lambda * (double)ssim_lambda / nS),
                     (float)((double)rgb_lambda * (1.0 - (double)ssim_lambda)), v_render, photo_sums);
  GSL_CHECK_LAUNCH();
  return GSL_OK;
}
