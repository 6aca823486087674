// Frame-to-map localisation: the rows of the map that a depth frame SEES THROUGH are removed, in map order
// (gsplatloc_amd/mapping.py: remove_seen_through).  A depth frame with a known pose says that nothing stands between
// the camera and the surface it observes: a live row that projects into the image and lies clearly in front of
// everything the frame observes around its pixel is a ghost -- a depth outlier, a badly placed edge, an object that
// has moved since -- and goes.
//
// Row i of means[n,3], projected to z, uf, vf (map_dev.h: the projection, the inside rule and the window):
//   tested  = z > near and inside;
//   blocked = some pixel of the window has a depth d that is not (finite and > 0), or not (z < d * keep) -- one
//             rounded product;
//   removed = tested and not blocked.
// Comparisons that are false for a NaN: NaN / inf rows, rows behind the camera or outside the image are untested and
// stay, a pixel without depth anywhere in the window keeps the row (no evidence, no removal).
//
// Order-preserving compaction (compact_dev.h), one row per thread.  The ballot records the rows that STAY, so what
// k_map_view_gather (map_view.hip, unchanged: same workspace layout) then moves are the survivors:
//   k_map_free_select  evaluates the rule and records it;
//   launch_count_scan  over the counts, total -> counters[0].
// 12 B read per row and up to (2 window + 1)^2 depth values from 2 window + 1 image lines; the map is in the raster
// order of its frames, so neighbouring lanes read neighbouring pixels.  The window is a runtime loop, one load in flight
// per lane (loading a line's pixels together was measured: 6.9 instead of 7.4 us at 375 k rows, within the spread of
// either, for twice the registers -- NOTES.md, "Free space").  No atomics, no LDS beyond the helper's.
#include "compact_dev.h"
#include "gsloc_internal.h"
#include "map_dev.h"

namespace gsl {

__global__ __launch_bounds__(COMPACT_THREADS) void k_map_free_select(
    const float* __restrict__ means, long long n_rows, const float* __restrict__ w2c, float fx, float fy, float cx,
    float cy, const float* __restrict__ depth, int width, int height, float u_last, float v_last, float keep, int window,
    float near_plane, uint64_t* __restrict__ ballots, uint32_t* __restrict__ block_counts,
    int32_t* __restrict__ counters) {
  const long long g = (long long)blockIdx.x * COMPACT_THREADS + threadIdx.x;
  if (g == 0) {  // the scan that follows in the stream writes [0]
    counters[1] = 0;
    counters[2] = 0;  // nothing gathered yet
  }
  bool stays = false;
  if (g < n_rows) {
    const MapPixel p = map_project(w2c, map_load_row(means, g), fx, fy, cx, cy);
    bool seen_through = p.z > near_plane && map_inside(p, u_last, v_last);
    if (seen_through) {
      const MapWindow win = map_window(p, window, width, height);
      for (int vv = win.v0; vv <= win.v1; ++vv) {
        const float* line = depth + (size_t)vv * (size_t)width;
        for (int uu = win.u0; uu <= win.u1; ++uu) {
          const float d = line[uu];
          seen_through = seen_through && d > 0.f && d < INFINITY && p.z < d * keep;
        }
      }
    }
    stays = !seen_through;
  }
  compact_record(stays, ballots, block_counts);
}

}  // namespace gsl

extern "C" int gsl_map_free_select(const float* means, int64_t n_rows, const float* w2c, float fx, float fy, float cx,
                                   float cy, const float* depth, int width, int height, float keep, int window_px,
                                   float near_plane, int32_t* counters, void* ws, size_t ws_bytes, void* stream) {
  if (!means || !w2c || !depth || !counters || !ws) return GSL_ERR_BAD_ARG;
  if (!gsl::map_rows_ok(n_rows) || !gsl::map_image_ok(width, height)) return GSL_ERR_BAD_ARG;
  if (!gsl::map_focal_ok(fx, fy) || !(keep > 0.f && keep <= 1.f)) return GSL_ERR_BAD_ARG;
  if (window_px < 0 || window_px > gsl::MAP_MAX_WINDOW) return GSL_ERR_BAD_ARG;
  if (ws_bytes < gsl_map_view_ws_bytes(n_rows)) return GSL_ERR_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  const int nb = (int)gsl::compact_blocks(n_rows);
  const gsl::CompactWs w = gsl::compact_ws(ws, nb);
  hipLaunchKernelGGL(gsl::k_map_free_select, dim3(nb), dim3(gsl::COMPACT_THREADS), 0, st, means, (long long)n_rows, w2c,
                     fx, fy, cx, cy, depth, width, height, (float)(width - 1), (float)(height - 1), keep, window_px,
                     near_plane, w.ballots, w.counts, counters);
  GSL_CHECK_LAUNCH();
  gsl::launch_count_scan(st, w.counts, nb, w.bases, counters);
  GSL_CHECK_LAUNCH();
  return GSL_OK;
}
