// Frame-to-map localisation: the rows of the map that a depth frame SEES THROUGH are removed, in map order
// (gsplatloc_amd/mapping.py: remove_seen_through).  A depth frame with a known pose says that nothing stands between
// the camera and the surface it observes: a live row that projects into the image and lies clearly in front of
// everything the frame observes around its pixel is a ghost -- a depth outlier, a badly placed edge, an object that
// has moved since -- and goes.
//
// Row i of means[n,3], with w the rows of w2c (world to camera, row-major):
//   x = ((w0 px + w1 py) + w2 pz) + w3, y and z likewise;  u = fx x / z + cx, v = fy y / z + cy;
//   uf = rintf(u), vf = rintf(v) (round half to even: depth_to_points puts pixel u at (u - cx) / fx, a pixel's own
//   point projects onto the integer u);
//   tested  = z > near and 0 <= uf <= width - 1 and 0 <= vf <= height - 1 (float comparisons, then the conversion;
//             rintf(-0.5) = -0 passes and is column 0);
//   blocked = some pixel (uf + du, vf + dv), |du|, |dv| <= window, INSIDE the image has a depth d that is not (finite
//             and > 0), or not (z < d * keep) -- one rounded product;
//   removed = tested and not blocked.
// float32, every operation rounded once in the order written (no contraction, correctly rounded division), comparisons
// that are false for a NaN: NaN / inf rows, rows behind the camera or outside the image are untested and stay, a pixel
// without depth anywhere in the window keeps the row (no evidence, no removal).  On given inputs the rule has no
// rounding freedom and the numpy mirror of the tests decides identically.
//
// Order-preserving compaction (compact_dev.h), one row per thread.  The ballot records the rows that STAY, so what
// k_map_view_gather (map_view.hip, unchanged: same workspace layout) then moves are the survivors:
//   k_map_free_select  evaluates the rule and records it;
//   launch_count_scan  over the counts, total -> counters[0].
// 12 B read per row and up to (2 window + 1)^2 depth values from 2 window + 1 image lines; the map is in the raster
// order of its frames, so neighbouring lanes read neighbouring pixels.  The window is a runtime loop, one load in flight
// per lane (loading a line's pixels together was measured: 6.9 instead of 7.4 us at 375 k rows, within the spread of
// either, for twice the registers -- NOTES.md, "Free space").  No atomics, no LDS beyond the helper's.
#include <math.h>

#include "compact_dev.h"
#include "gsloc_internal.h"

namespace gsl {

constexpr int MAX_WINDOW = 3;  // window_px is 0 .. MAX_WINDOW (the entry point refuses anything else)

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
#pragma clang fp contract(off)
    const float px = means[3 * (size_t)g], py = means[3 * (size_t)g + 1], pz = means[3 * (size_t)g + 2];
    const float x = ((w2c[0] * px + w2c[1] * py) + w2c[2] * pz) + w2c[3];
    const float y = ((w2c[4] * px + w2c[5] * py) + w2c[6] * pz) + w2c[7];
    const float z = ((w2c[8] * px + w2c[9] * py) + w2c[10] * pz) + w2c[11];
    const float u = fx * x / z + cx, v = fy * y / z + cy;
    const float uf = rintf(u), vf = rintf(v);
    bool seen_through = z > near_plane && uf >= 0.f && uf <= u_last && vf >= 0.f && vf <= v_last;
    if (seen_through) {  // uf, vf are integers in [0, width - 1] x [0, height - 1]: every index below is inside
      const int uc = (int)uf, vc = (int)vf;
      const int u0 = uc - window > 0 ? uc - window : 0, u1 = uc + window < width - 1 ? uc + window : width - 1;
      const int v0 = vc - window > 0 ? vc - window : 0, v1 = vc + window < height - 1 ? vc + window : height - 1;
      for (int vv = v0; vv <= v1; ++vv) {
        const float* line = depth + (size_t)vv * (size_t)width;
        for (int uu = u0; uu <= u1; ++uu) {
          const float d = line[uu];
          seen_through = seen_through && d > 0.f && d < INFINITY && z < d * keep;
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
  if (n_rows <= 0 || n_rows >= 0x80000000ll) return GSL_ERR_BAD_ARG;  // 32-bit counts and indices
  if (width <= 0 || height <= 0 || (long long)width * height > 0x7fffffffll) return GSL_ERR_BAD_ARG;
  if (!(fx != 0.f) || !(fy != 0.f) || !(keep > 0.f && keep <= 1.f)) return GSL_ERR_BAD_ARG;
  if (window_px < 0 || window_px > gsl::MAX_WINDOW) return GSL_ERR_BAD_ARG;
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
