// Frame-to-map localisation: the pixels of a depth frame that the map does not explain yet are back-projected and
// appended to the map's point arrays (gsplatloc_amd/mapping.py), in raster order.
//
// A pixel is NEW when its observed depth d_o is finite and > 0 and (the map's rendered alpha there is below alpha_min,
// or d_o < d_r * keep with d_r the map's rendered expected depth and keep = 1 - depth_rho: a surface in front of what the
// map shows).  The rule is evaluated in float32 with one rounded product and comparisons only -- no contraction -- so on
// given inputs it has no rounding freedom and the numpy mirror of the tests selects the same pixels.
//
// Order-preserving compaction, the structure of project_packed.hip for the same reason (no workgroup waits for another
// one: a look-back scan or a "last workgroup" ticket needs device-scope release/acquire across the eight XCD L2s,
// NOTES.md round 3; atomics would make the order run-dependent).  One pixel per thread, 256-thread workgroups:
//   k_map_select   evaluates the rule; one 64-bit ballot per wave, one count per workgroup;
//   launch_count_scan (project_packed.hip)  exclusive scan of the workgroup counts, total -> n_new[0];
//   k_map_append   the lanes whose ballot bit is set back-project their pixel and store it at
//                  n_live + workgroup base + selected lanes of the earlier waves + mbcnt; rows at or beyond the
//                  capacity are dropped, the number stored -> n_new[1].
// The fill pass takes its positions from the stored ballots alone.  Memory-streaming: 12 B read per pixel in the first
// pass, 16 B read and 24 B written per selected pixel in the second.
#include "gsloc_internal.h"

namespace gsl {

__global__ __launch_bounds__(256) void k_map_select(const float* __restrict__ render_depth,
                                                    const float* __restrict__ alphas, const float* __restrict__ depth,
                                                    long long n_px, float alpha_min, float keep,
                                                    uint64_t* __restrict__ ballots, uint32_t* __restrict__ block_counts) {
  const long long g = (long long)blockIdx.x * 256 + threadIdx.x;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  bool is_new = false;
  if (g < n_px) {
#pragma clang fp contract(off)
    const float d_o = depth[g];
    is_new = d_o > 0.f && d_o <= 3.40282347e+38f;  // finite and positive (false for a NaN)
    if (is_new && render_depth != nullptr) {
      const float a = alphas[g], limit = render_depth[g] * keep;
      is_new = a < alpha_min || d_o < limit;
    }
  }
  const unsigned long long sel = __ballot(is_new);
  __shared__ uint32_t cnt[4];
  if (lane == 0) {
    ballots[(size_t)blockIdx.x * 4 + wv] = sel;
    cnt[wv] = (uint32_t)__popcll(sel);
  }
  __syncthreads();
  if (threadIdx.x == 0) block_counts[blockIdx.x] = cnt[0] + cnt[1] + cnt[2] + cnt[3];
}

__global__ __launch_bounds__(256) void k_map_append(const float* __restrict__ depth, const float* __restrict__ rgb,
                                                    int W, long long n_px, float fx, float fy, float cx, float cy,
                                                    const float* __restrict__ c2w, const uint64_t* __restrict__ ballots,
                                                    const uint32_t* __restrict__ block_bases, float* __restrict__ means,
                                                    float* __restrict__ colors, long long n_live, long long capacity,
                                                    int32_t* __restrict__ n_new) {
  const long long g = (long long)blockIdx.x * 256 + threadIdx.x;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const long long room = capacity - n_live;
  if (g == 0) {
    const long long selected = n_new[0];
    n_new[1] = (int32_t)(selected < room ? selected : room);
  }
  // position: rows of earlier workgroups, of earlier waves of this one, of lower lanes of this wave
  const unsigned long long sel = ballots[(size_t)blockIdx.x * 4 + wv];
  long long pos = block_bases[blockIdx.x];
  for (int w = 0; w < wv; ++w) pos += __popcll(ballots[(size_t)blockIdx.x * 4 + w]);
  pos += __builtin_amdgcn_mbcnt_hi((uint32_t)(sel >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)sel, 0u));
  if (g >= n_px || !((sel >> lane) & 1ull) || pos >= room) return;
  const int v = (int)(g / W), u = (int)(g - (long long)v * W);
  const float d_o = depth[g];
  const float r = rgb[3 * (size_t)g], gr = rgb[3 * (size_t)g + 1], b = rgb[3 * (size_t)g + 2];
  const size_t row = (size_t)(n_live + pos);
  {
#pragma clang fp contract(off)
    // depth_to_points: (u - cx) / fx * d, (v - cy) / fy * d, d; then R p + t
    const float x = ((float)u - cx) / fx * d_o, y = ((float)v - cy) / fy * d_o;
#pragma unroll
    for (int j = 0; j < 3; ++j)
      means[3 * row + j] = ((c2w[4 * j] * x + c2w[4 * j + 1] * y) + c2w[4 * j + 2] * d_o) + c2w[4 * j + 3];
    colors[3 * row] = r / 255.f;
    colors[3 * row + 1] = gr / 255.f;
    colors[3 * row + 2] = b / 255.f;
  }
}

static inline long long map_blocks(int width, int height) { return ((long long)width * height + 255) / 256; }

}  // namespace gsl

extern "C" size_t gsl_map_ws_bytes(int width, int height) {
  // [ballots nb x 4 uint64][block counts nb uint32][block bases nb uint32]
  long long nb = (width > 0 && height > 0) ? gsl::map_blocks(width, height) : 0;
  if (nb < 1) nb = 1;
  return (size_t)nb * (4 * sizeof(uint64_t) + 2 * sizeof(uint32_t));
}

// Argument checks shared by the two passes.
static int map_check(const float* depth, int width, int height, const int32_t* n_new, const void* ws, size_t ws_bytes) {
  if (width <= 0 || height <= 0 || (long long)width * height > 0x7FFFFFFFll) return GSL_ERR_BAD_ARG;  // 32-bit counts
  if (!depth || !n_new || !ws || ws_bytes < gsl_map_ws_bytes(width, height)) return GSL_ERR_BAD_ARG;
  return GSL_OK;
}

extern "C" int gsl_map_select(const float* render_depth, const float* alphas, const float* depth, int width, int height,
                              float alpha_min, float keep, int32_t* n_new, void* ws, size_t ws_bytes, void* stream) {
  int rc = map_check(depth, width, height, n_new, ws, ws_bytes);
  if (rc != GSL_OK) return rc;
  if ((render_depth == nullptr) != (alphas == nullptr)) return GSL_ERR_BAD_ARG;  // both, or the "no render yet" form
  hipStream_t st = (hipStream_t)stream;
  const int nb = (int)gsl::map_blocks(width, height);
  uint64_t* ballots = (uint64_t*)ws;
  uint32_t* counts = (uint32_t*)(ballots + (size_t)nb * 4);
  uint32_t* bases = counts + nb;
  if (gsl::zero_u32(n_new + 1, 1, st) != GSL_OK) return GSL_ERR_HIP;  // nothing appended yet
  hipLaunchKernelGGL(gsl::k_map_select, dim3(nb), dim3(256), 0, st, render_depth, alphas, depth,
                     (long long)width * height, alpha_min, keep, ballots, counts);
  GSL_CHECK_LAUNCH();
  gsl::launch_count_scan(st, counts, nb, bases, n_new);
  GSL_CHECK_LAUNCH();
  return GSL_OK;
}

extern "C" int gsl_map_append(const float* depth, const float* rgb, int width, int height, float fx, float fy, float cx,
                              float cy, const float* c2w, float* means, float* colors, int64_t n_live, int64_t capacity,
                              int32_t* n_new, void* ws, size_t ws_bytes, void* stream) {
  int rc = map_check(depth, width, height, n_new, ws, ws_bytes);
  if (rc != GSL_OK) return rc;
  if (!rgb || !c2w || !means || !colors) return GSL_ERR_BAD_ARG;
  if (capacity <= 0 || n_live < 0 || n_live > capacity) return GSL_ERR_BAD_ARG;
  if (!(fx != 0.f) || !(fy != 0.f)) return GSL_ERR_BAD_ARG;
  const int nb = (int)gsl::map_blocks(width, height);
  const uint64_t* ballots = (const uint64_t*)ws;
  const uint32_t* bases = (const uint32_t*)(ballots + (size_t)nb * 4) + nb;
  hipLaunchKernelGGL(gsl::k_map_append, dim3(nb), dim3(256), 0, (hipStream_t)stream, depth, rgb, width,
                     (long long)width * height, fx, fy, cx, cy, c2w, ballots, bases, means, colors, (long long)n_live,
                     (long long)capacity, n_new);
  GSL_CHECK_LAUNCH();
  return GSL_OK;
}
