// Frame-to-map localisation: the pixels of a depth frame that the map does not explain yet are back-projected and
// appended to the map's point arrays (gsplatloc_amd/mapping.py), in raster order.
//
// A pixel is NEW when its observed depth d_o is finite and > 0 and (the map's rendered alpha there is below alpha_min,
// or d_o < d_r * keep with d_r the map's rendered expected depth and keep = 1 - depth_rho: a surface in front of what the
// map shows).  The rule is evaluated in float32 with one rounded product and comparisons only -- no contraction -- so on
// given inputs it has no rounding freedom and the numpy mirror of the tests selects the same pixels.
//
// Order-preserving compaction (compact_dev.h), one pixel per thread:
//   k_map_select   evaluates the rule and records it; the scan's total -> n_new[0];
//   k_map_append   the lanes whose ballot bit is set back-project their pixel and store it at n_live + their position;
//                  rows at or beyond the capacity are dropped, the number stored -> n_new[1].
// Memory-streaming: 12 B read per pixel in the first pass, 16 B read and 24 B written per selected pixel in the second.
#include "compact_dev.h"
#include "gsloc_internal.h"
#include "map_dev.h"

namespace gsl {

__global__ __launch_bounds__(COMPACT_THREADS) void k_map_select(
    const float* __restrict__ render_depth, const float* __restrict__ alphas, const float* __restrict__ depth,
    long long n_px, float alpha_min, float keep, uint64_t* __restrict__ ballots, uint32_t* __restrict__ block_counts) {
  const long long g = (long long)blockIdx.x * COMPACT_THREADS + threadIdx.x;
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
  compact_record(is_new, ballots, block_counts);
}

__global__ __launch_bounds__(COMPACT_THREADS) void k_map_append(
    const float* __restrict__ depth, const float* __restrict__ rgb, int W, long long n_px, float fx, float fy, float cx,
    float cy, const float* __restrict__ c2w, const uint64_t* __restrict__ ballots,
    const uint32_t* __restrict__ block_bases, float* __restrict__ means, float* __restrict__ colors, long long n_live,
    long long capacity, int32_t* __restrict__ n_new) {
  const long long g = (long long)blockIdx.x * COMPACT_THREADS + threadIdx.x;
  const long long room = capacity - n_live;
  compact_store_clamped(n_new, room, n_new + 1);
  if (g >= n_px) return;
  const long long pos = compact_position(ballots, block_bases);
  if (!compact_kept(ballots) || pos >= room) return;
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

}  // namespace gsl

extern "C" size_t gsl_map_ws_bytes(int width, int height) {
  return gsl::compact_ws_bytes((width > 0 && height > 0) ? (long long)width * height : 0);
}

// Argument checks shared by the two passes.
static int map_check(const float* depth, int width, int height, const int32_t* n_new, const void* ws, size_t ws_bytes) {
  if (!gsl::map_image_ok(width, height)) return GSL_ERR_BAD_ARG;
  if (!depth || !n_new || !ws || ws_bytes < gsl_map_ws_bytes(width, height)) return GSL_ERR_BAD_ARG;
  return GSL_OK;
}

extern "C" int gsl_map_select(const float* render_depth, const float* alphas, const float* depth, int width, int height,
                              float alpha_min, float keep, int32_t* n_new, void* ws, size_t ws_bytes, void* stream) {
  int rc = map_check(depth, width, height, n_new, ws, ws_bytes);
  if (rc != GSL_OK) return rc;
  if ((render_depth == nullptr) != (alphas == nullptr)) return GSL_ERR_BAD_ARG;  // both, or the "no render yet" form
  hipStream_t st = (hipStream_t)stream;
  const int nb = (int)gsl::compact_blocks((long long)width * height);
  const gsl::CompactWs w = gsl::compact_ws(ws, nb);
  if (gsl::zero_u32(n_new + 1, 1, st) != GSL_OK) return GSL_ERR_HIP;  // nothing appended yet
  hipLaunchKernelGGL(gsl::k_map_select, dim3(nb), dim3(gsl::COMPACT_THREADS), 0, st, render_depth, alphas, depth,
                     (long long)width * height, alpha_min, keep, w.ballots, w.counts);
  GSL_CHECK_LAUNCH();
  gsl::launch_count_scan(st, w.counts, nb, w.bases, n_new);
  GSL_CHECK_LAUNCH();
  return GSL_OK;
}

extern "C" int gsl_map_append(const float* depth, const float* rgb, int width, int height, float fx, float fy, float cx,
                              float cy, const float* c2w, float* means, float* colors, int64_t n_live, int64_t capacity,
                              int32_t* n_new, void* ws, size_t ws_bytes, void* stream) {
  int rc = map_check(depth, width, height, n_new, ws, ws_bytes);
  if (rc != GSL_OK) return rc;
  if (!rgb || !c2w || !means || !colors) return GSL_ERR_BAD_ARG;
  if (capacity <= 0 || n_live < 0 || n_live > capacity || !gsl::map_focal_ok(fx, fy)) return GSL_ERR_BAD_ARG;
  const int nb = (int)gsl::compact_blocks((long long)width * height);
  const gsl::CompactWs w = gsl::compact_ws(ws, nb);
  hipLaunchKernelGGL(gsl::k_map_append, dim3(nb), dim3(gsl::COMPACT_THREADS), 0, (hipStream_t)stream, depth, rgb,
                     width, (long long)width * height, fx, fy, cx, cy, c2w, w.ballots, w.bases, means, colors,
                     (long long)n_live, (long long)capacity, n_new);
  GSL_CHECK_LAUNCH();
  return GSL_OK;
}
