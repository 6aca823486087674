// Frame-to-map localisation: the rows of the map that are IN VIEW from a pose -- inside the image widened by a guard
// band of guard_px pixels, between the depth planes -- are compacted, in map order, into a working set that the tracker
// sees instead of the whole map (gsplatloc_amd/mapping.py: select_view / view_violations).
//
// Row i of means[n,3] is in view when it is in the band (map_dev.h: the projection and the band rule) with lo = -guard:
//   z > near and z < far;  -guard <= u <= (width - 1) + guard,  -guard <= v <= (height - 1) + guard.
//
// Order-preserving compaction (compact_dev.h), one row per thread; the order is the map's in every run:
//   k_map_view_select  evaluates the rule and records it -- and, given the ballots an earlier call left for the same
//                      rows (prev), a second count per workgroup: the rows in view now whose bit was clear then;
//   launch_count_scan  over the counts, total -> counters[0]; a second one over the second counts, total ->
//                      counters[1] (the counts and their bases are the two extra columns of ws; the bases are scratch);
//   k_map_view_gather  the lanes whose ballot bit is set copy their mean, colour and index to their position; rows at
//                      or beyond out_capacity are dropped, the number stored -> counters[2].
// Memory-streaming: 12 B read per row in the first pass, 24 B read and 24 - 28 B written per selected row in the second.
#include "compact_dev.h"
#include "gsloc_internal.h"
#include "map_dev.h"

namespace gsl {

__global__ __launch_bounds__(COMPACT_THREADS) void k_map_view_select(
    const float* __restrict__ means, long long n_rows, const float* __restrict__ w2c, float fx, float fy, float cx,
    float cy, float guard_lo, float u_hi, float v_hi, float near_plane, float far_plane,
    const uint64_t* __restrict__ prev_ballots, uint64_t* __restrict__ ballots, uint32_t* __restrict__ block_counts,
    uint32_t* __restrict__ block_fresh, int32_t* __restrict__ counters) {
  const long long g = (long long)blockIdx.x * COMPACT_THREADS + threadIdx.x;
  if (g == 0) {  // the scans that follow in the stream write [0] and, with prev, [1]
    if (prev_ballots == nullptr) counters[1] = 0;
    counters[2] = 0;  // nothing gathered yet
  }
  bool in_view = false;
  if (g < n_rows)
    in_view = map_in_band(map_project(w2c, map_load_row(means, g), fx, fy, cx, cy), near_plane, far_plane, guard_lo,
                          u_hi, v_hi);
  const unsigned long long sel = compact_ballot(in_view, ballots);
  // second mask: in view now, bit clear in prev
  const unsigned long long mask[2] = {sel, prev_ballots ? sel & ~prev_ballots[compact_wave_slot()] : 0ull};
  uint32_t sum[2];
  if (compact_block_sums(mask, sum)) {
    block_counts[blockIdx.x] = sum[0];
    if (prev_ballots) block_fresh[blockIdx.x] = sum[1];
  }
}

__global__ __launch_bounds__(COMPACT_THREADS) void k_map_view_gather(
    const float* __restrict__ means, const float* __restrict__ colors, long long n_rows,
    const uint64_t* __restrict__ ballots, const uint32_t* __restrict__ block_bases, float* __restrict__ out_means,
    float* __restrict__ out_colors, int32_t* __restrict__ out_ids, long long out_capacity,
    int32_t* __restrict__ counters) {
  const long long g = (long long)blockIdx.x * COMPACT_THREADS + threadIdx.x;
  compact_store_clamped(counters, out_capacity, counters + 2);
  if (g >= n_rows) return;
  const long long pos = compact_position(ballots, block_bases);
  if (!compact_kept(ballots) || pos >= out_capacity) return;
  const size_t src = 3 * (size_t)g, dst = 3 * (size_t)pos;
  const float m0 = means[src], m1 = means[src + 1], m2 = means[src + 2];
  const float c0 = colors[src], c1 = colors[src + 1], c2 = colors[src + 2];
  out_means[dst] = m0;
  out_means[dst + 1] = m1;
  out_means[dst + 2] = m2;
  out_colors[dst] = c0;
  out_colors[dst + 1] = c1;
  out_colors[dst + 2] = c2;
  if (out_ids) out_ids[pos] = (int32_t)g;
}

}  // namespace gsl

extern "C" size_t gsl_map_view_ws_bytes(int64_t n_rows) {
  // two extra columns: the second counts and their bases
  return gsl::compact_ws_bytes(n_rows < 0x80000000ll ? (long long)n_rows : 0, 2);
}

// Argument checks shared by the two passes.
static int view_check(const float* means, int64_t n_rows, const int32_t* counters, const void* ws, size_t ws_bytes) {
  if (!gsl::map_rows_ok(n_rows)) return GSL_ERR_BAD_ARG;
  if (!means || !counters || !ws) return GSL_ERR_BAD_ARG;
  if (ws_bytes < gsl_map_view_ws_bytes(n_rows)) return GSL_ERR_WORKSPACE;
  return GSL_OK;
}

extern "C" int gsl_map_view_select(const float* means, int64_t n_rows, const float* w2c, float fx, float fy, float cx,
                                   float cy, int width, int height, float guard_px, float near_plane, float far_plane,
                                   const void* prev_ws, int32_t* counters, void* ws, size_t ws_bytes, void* stream) {
  if (!w2c || width <= 0 || height <= 0 || !gsl::map_focal_ok(fx, fy)) return GSL_ERR_BAD_ARG;
  if (!(guard_px >= 0.f) || !(near_plane < far_plane) || (prev_ws != nullptr && prev_ws == ws)) return GSL_ERR_BAD_ARG;
  int rc = view_check(means, n_rows, counters, ws, ws_bytes);
  if (rc != GSL_OK) return rc;
  hipStream_t st = (hipStream_t)stream;
  const int nb = (int)gsl::compact_blocks(n_rows);
  const gsl::CompactWs w = gsl::compact_ws(ws, nb);
  uint32_t *fresh = w.extra, *fresh_bases = w.extra + nb;
  const float u_hi = (float)(width - 1) + guard_px, v_hi = (float)(height - 1) + guard_px;  // one float32 sum each
  hipLaunchKernelGGL(gsl::k_map_view_select, dim3(nb), dim3(gsl::COMPACT_THREADS), 0, st, means, (long long)n_rows,
                     w2c, fx, fy, cx, cy, -guard_px, u_hi, v_hi, near_plane, far_plane, (const uint64_t*)prev_ws,
                     w.ballots, w.counts, fresh, counters);
  GSL_CHECK_LAUNCH();
  gsl::launch_count_scan(st, w.counts, nb, w.bases, counters);
  GSL_CHECK_LAUNCH();
  if (prev_ws) {
    gsl::launch_count_scan(st, fresh, nb, fresh_bases, counters + 1);
    GSL_CHECK_LAUNCH();
  }
  return GSL_OK;
}

extern "C" int gsl_map_view_gather(const float* means, const float* colors, int64_t n_rows, float* out_means,
                                   float* out_colors, int32_t* out_ids, int64_t out_capacity, int32_t* counters,
                                   void* ws, size_t ws_bytes, void* stream) {
  if (!colors || !out_means || !out_colors || out_capacity < 0) return GSL_ERR_BAD_ARG;
  int rc = view_check(means, n_rows, counters, ws, ws_bytes);
  if (rc != GSL_OK) return rc;
  const int nb = (int)gsl::compact_blocks(n_rows);
  const gsl::CompactWs w = gsl::compact_ws(ws, nb);
  hipLaunchKernelGGL(gsl::k_map_view_gather, dim3(nb), dim3(gsl::COMPACT_THREADS), 0, (hipStream_t)stream, means,
                     colors, (long long)n_rows, w.ballots, w.bases, out_means, out_colors, out_ids,
                     (long long)out_capacity, counters);
  GSL_CHECK_LAUNCH();
  return GSL_OK;
}
