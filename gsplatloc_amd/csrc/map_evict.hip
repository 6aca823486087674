// Frame-to-map localisation: a map that lives in bounded memory (gsplatloc_amd/mapping.py: observe / evict).  Every row
// carries the index of the last frame that OBSERVED it -- it projects into the frame, or into the band around it in
// which a centre still paints into the image, and where there is a depth to hold it against it lies on the observed
// surface -- and when a frame's new rows do not fit, exactly as many rows as are needed go: the least recently observed
// first, in map order among rows of the same age.
//
// gsl_map_observe, one row per thread.  Row i of means[n,3], projected to z, u, v, uf, vf (map_dev.h: the projection,
// the band rule, the inside rule and the window):
//   in reach = in the band with lo = -reach: the view rule of map_view.hip with guard = reach;
//   agrees   = some pixel of the window has a depth d that is finite and > 0 with z >= d * keep and z * keep <= d --
//              two rounded products, no division;
//   observed = in reach and (not inside or agrees):  stamps[i] = now.  Every other row keeps its stamp.
// Comparisons that are false for a NaN: NaN / inf rows are never observed.
// 12 B read per row, up to (2 window + 1)^2 depth values, one conditional 4 B store; no LDS, no atomics.
//
// gsl_map_evict_select, all in integers.  age = clamp(now - stamp, 0, 1023); a row is evictable when age >= min_age;
// E = min(need, evictable rows); a* = the largest age with count(age >= a*) >= E.  Evicted: every row with age > a*,
// and of the rows with age == a* the first E - count(age > a*) (the tie quota) in map order.  The launches:
//   zero_u32             the 1024 bins;
//   k_map_age_hist       a histogram per workgroup in LDS (4 KB, ds_add_u32), its non-empty bins added to the bins in
//                        memory with one integer atomic each -- integer sums do not depend on the order;
//   k_map_age_threshold  one workgroup: the suffix sums of the bins from 1023 down -> a*, the tie quota and E;
//   k_map_age_ties       the ballot and the workgroup count of age == a* (compact_dev.h);
//   launch_count_scan    over the tie counts;
//   k_map_evict_select   the age again; a tie's rank among the ties is its compact_position on the tie ballots; the rows
//                        that STAY are recorded in the head of ws, the layout of gsl_map_view_select, so that
//                        gsl_map_view_gather (map_view.hip, unchanged) moves the survivors;
//   launch_count_scan    over the counts of the rows that stay, total -> counters[0].
// Ages cluster -- the rows of a frame share a stamp -- so most lanes of a wave add to one bin: 64 ds_add on one address
// were measured faster than a readlane / ballot aggregation loop (NOTES.md, round 4 dead ends), the plain form stands.
//
// ws = [head: gsl_map_view_ws_bytes(n) -- ballots of the rows that stay nb x 4 uint64, counts nb, bases nb, tie counts
//       nb, tie bases nb][tie ballots nb x 4 uint64][bins 1024 uint32][a*, tie quota, E, rows of age a*] (uint32).
#include "compact_dev.h"
#include "gsloc_internal.h"
#include "map_dev.h"

namespace gsl {

constexpr int AGE_BINS = 1024;  // ages are clamped to 0 .. AGE_BINS - 1
constexpr int HIST_THREADS = 256;
constexpr int HIST_ROWS = 2048;  // rows per workgroup of k_map_age_hist: eight per thread, one clear and one flush
constexpr int EVICT_PARAMS = 4;  // a*, tie quota, E, rows of age a*

struct EvictWs {
  CompactWs head;  // extra columns: tie counts, tie bases
  uint64_t* tie_ballots;
  uint32_t *bins, *params;
};
static inline size_t evict_ws_bytes(long long n) {
  const long long nb = n > 0 ? compact_blocks(n) : 1;
  return compact_ws_bytes(n, 2) + (size_t)nb * COMPACT_WAVES * sizeof(uint64_t) +
         (size_t)(AGE_BINS + EVICT_PARAMS) * sizeof(uint32_t);
}
static inline EvictWs evict_ws(void* ws, long long n, int nb) {
  EvictWs w;
  w.head = compact_ws(ws, nb);
  w.tie_ballots = (uint64_t*)((char*)ws + compact_ws_bytes(n, 2));  // 48 nb bytes in: aligned for uint64
  w.bins = (uint32_t*)(w.tie_ballots + (size_t)nb * COMPACT_WAVES);
  w.params = w.bins + AGE_BINS;
  return w;
}

__device__ static inline int age_of(int32_t now, int32_t stamp) {
  const long long a = (long long)now - (long long)stamp;  // no 32-bit overflow whatever the stamp holds
  return a < 0 ? 0 : a > AGE_BINS - 1 ? AGE_BINS - 1 : (int)a;
}

__global__ __launch_bounds__(COMPACT_THREADS) void k_map_observe(
    const float* __restrict__ means, long long n_rows, const float* __restrict__ w2c, float fx, float fy, float cx,
    float cy, const float* __restrict__ depth, int width, int height, float u_last, float v_last, float keep, int window,
    float reach_lo, float u_hi, float v_hi, float near_plane, float far_plane, int32_t now,
    int32_t* __restrict__ stamps) {
  const long long g = (long long)blockIdx.x * COMPACT_THREADS + threadIdx.x;
  if (g >= n_rows) return;
  const MapPixel p = map_project(w2c, map_load_row(means, g), fx, fy, cx, cy);
  if (!map_in_band(p, near_plane, far_plane, reach_lo, u_hi, v_hi)) return;
  bool observed = true;  // in the band around the image: it paints into the frame, there is no depth to hold it against
  if (map_inside(p, u_last, v_last)) {
    const MapWindow win = map_window(p, window, width, height);
    const float zk = p.z * keep;
    observed = false;
    for (int vv = win.v0; vv <= win.v1; ++vv) {
      const float* line = depth + (size_t)vv * (size_t)width;
      for (int uu = win.u0; uu <= win.u1; ++uu) {
        const float d = line[uu];
        observed = observed || (d > 0.f && d < INFINITY && p.z >= d * keep && zk <= d);
      }
    }
  }
  if (observed) stamps[g] = now;
}

__global__ __launch_bounds__(HIST_THREADS) void k_map_age_hist(const int32_t* __restrict__ stamps, long long n_rows,
                                                              int32_t now, uint32_t* __restrict__ bins) {
  __shared__ uint32_t local[AGE_BINS];
  for (int b = threadIdx.x; b < AGE_BINS; b += HIST_THREADS) local[b] = 0u;
  __syncthreads();
  const long long first = (long long)blockIdx.x * HIST_ROWS;
  const long long end = first + HIST_ROWS < n_rows ? first + HIST_ROWS : n_rows;
  for (long long g = first + threadIdx.x; g < end; g += HIST_THREADS) atomicAdd(&local[age_of(now, stamps[g])], 1u);
  __syncthreads();
  for (int b = threadIdx.x; b < AGE_BINS; b += HIST_THREADS) {
    const uint32_t c = local[b];
    if (c != 0u) atomicAdd(&bins[b], c);
  }
}

// One workgroup; thread t owns the bins 4 t .. 4 t + 3.  at_least(a) = rows with age >= a, non-increasing in a, so
// exactly one age has at_least(a) >= E and (a == 1023 or at_least(a + 1) < E): that is a*.
__global__ __launch_bounds__(HIST_THREADS) void k_map_age_threshold(const uint32_t* __restrict__ bins, int min_age,
                                                                   long long need, uint32_t* __restrict__ params) {
  constexpr int PER = AGE_BINS / HIST_THREADS;
  __shared__ uint32_t above[HIST_THREADS];  // rows in the bins of the threads after this one
  __shared__ uint32_t evictable;
  uint32_t mine[PER], sum = 0;
#pragma unroll
  for (int k = 0; k < PER; ++k) {
    mine[k] = bins[PER * threadIdx.x + k];
    sum += mine[k];
  }
  above[threadIdx.x] = sum;
  if (threadIdx.x == 0) evictable = 0u;  // min_age beyond the last bin: nothing is that old
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t run = 0;
    for (int t = HIST_THREADS - 1; t >= 0; --t) {
      const uint32_t s = above[t];
      above[t] = run;
      run += s;
    }
  }
  __syncthreads();
  uint32_t at_least[PER + 1];  // at_least[k]: rows with age >= 4 t + k
  at_least[PER] = above[threadIdx.x];
#pragma unroll
  for (int k = PER - 1; k >= 0; --k) at_least[k] = at_least[k + 1] + mine[k];
#pragma unroll
  for (int k = 0; k < PER; ++k)
    if (PER * (int)threadIdx.x + k == min_age) evictable = at_least[k];
  __syncthreads();
  const long long ev = evictable;
  const uint32_t E = (uint32_t)(need < ev ? need : ev);
#pragma unroll
  for (int k = 0; k < PER; ++k) {
    const int a = PER * (int)threadIdx.x + k;
    if (at_least[k] >= E && (a == AGE_BINS - 1 || at_least[k + 1] < E)) {
      params[0] = (uint32_t)a;
      params[1] = E - (a == AGE_BINS - 1 ? 0u : at_least[k + 1]);  // the ties that go: E - rows older than a*
      params[2] = E;
    }
  }
}

__global__ __launch_bounds__(COMPACT_THREADS) void k_map_age_ties(const int32_t* __restrict__ stamps, long long n_rows,
                                                                 int32_t now, const uint32_t* __restrict__ params,
                                                                 uint64_t* __restrict__ tie_ballots,
                                                                 uint32_t* __restrict__ tie_counts) {
  const long long g = (long long)blockIdx.x * COMPACT_THREADS + threadIdx.x;
  const bool tie = g < n_rows && age_of(now, stamps[g]) == (int)params[0];
  compact_record(tie, tie_ballots, tie_counts);
}

__global__ __launch_bounds__(COMPACT_THREADS) void k_map_evict_select(
    const int32_t* __restrict__ stamps, long long n_rows, int32_t now, const uint32_t* __restrict__ params,
    const uint64_t* __restrict__ tie_ballots, const uint32_t* __restrict__ tie_bases, uint64_t* __restrict__ ballots,
    uint32_t* __restrict__ block_counts, int32_t* __restrict__ counters) {
  const long long g = (long long)blockIdx.x * COMPACT_THREADS + threadIdx.x;
  if (g == 0) {  // the scan that follows in the stream writes [0]
    counters[1] = (int32_t)params[2];
    counters[2] = 0;  // nothing gathered yet
  }
  bool stays = false;
  if (g < n_rows) {
    const int age = age_of(now, stamps[g]), oldest_kept = (int)params[0];
    // a tie's rank: the ties of earlier workgroups, of earlier waves, of lower lanes
    const bool goes = age > oldest_kept ||
                      (age == oldest_kept && compact_position(tie_ballots, tie_bases) < (long long)params[1]);
    stays = !goes;
  }
  compact_record(stays, ballots, block_counts);
}

__global__ __launch_bounds__(256) void k_map_gather_i32(const int32_t* __restrict__ src, long long n_src,
                                                       const int32_t* __restrict__ ids, long long n_ids,
                                                       int32_t* __restrict__ dst) {
  const long long r = (long long)blockIdx.x * 256 + threadIdx.x;
  if (r >= n_ids) return;
  const long long id = ids[r];
  dst[r] = id >= 0 && id < n_src ? src[id] : 0;  // an id outside the source: 0, nothing is read there
}

}  // namespace gsl

extern "C" int gsl_map_observe(const float* means, int64_t n_rows, const float* w2c, float fx, float fy, float cx,
                               float cy, const float* depth, int width, int height, float keep, int window_px,
                               float reach_px, float near_plane, float far_plane, int now, int32_t* stamps,
                               void* stream) {
  if (!means || !w2c || !depth || !stamps) return GSL_ERR_BAD_ARG;
  if (!gsl::map_rows_ok(n_rows) || !gsl::map_image_ok(width, height)) return GSL_ERR_BAD_ARG;
  if (!gsl::map_focal_ok(fx, fy) || !(keep > 0.f && keep <= 1.f)) return GSL_ERR_BAD_ARG;
  if (window_px < 0 || window_px > gsl::MAP_MAX_WINDOW) return GSL_ERR_BAD_ARG;
  if (!(reach_px >= 0.f) || !(near_plane < far_plane)) return GSL_ERR_BAD_ARG;
  const int nb = (int)gsl::compact_blocks(n_rows);
  const float u_hi = (float)(width - 1) + reach_px, v_hi = (float)(height - 1) + reach_px;  // one float32 sum each
  hipLaunchKernelGGL(gsl::k_map_observe, dim3(nb), dim3(gsl::COMPACT_THREADS), 0, (hipStream_t)stream, means,
                     (long long)n_rows, w2c, fx, fy, cx, cy, depth, width, height, (float)(width - 1),
                     (float)(height - 1), keep, window_px, -reach_px, u_hi, v_hi, near_plane, far_plane, now, stamps);
  GSL_CHECK_LAUNCH();
  return GSL_OK;
}

extern "C" size_t gsl_map_evict_ws_bytes(int64_t n_rows) {
  return gsl::evict_ws_bytes(n_rows < 0x80000000ll ? (long long)n_rows : 0);
}

extern "C" int gsl_map_evict_select(const int32_t* stamps, int64_t n_rows, int now, int min_age, int64_t need,
                                    int32_t* counters, void* ws, size_t ws_bytes, void* stream) {
  if (!stamps || !counters || !ws) return GSL_ERR_BAD_ARG;
  if (!gsl::map_rows_ok(n_rows)) return GSL_ERR_BAD_ARG;
  if (need < 0 || min_age < 1) return GSL_ERR_BAD_ARG;
  if (ws_bytes < gsl_map_evict_ws_bytes(n_rows)) return GSL_ERR_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  const int nb = (int)gsl::compact_blocks(n_rows);
  const gsl::EvictWs w = gsl::evict_ws(ws, (long long)n_rows, nb);
  uint32_t *tie_counts = w.head.extra, *tie_bases = w.head.extra + nb;
  int rc = gsl::zero_u32(w.bins, gsl::AGE_BINS, st);
  if (rc != GSL_OK) return rc;
  const int hist_blocks = (int)((n_rows + gsl::HIST_ROWS - 1) / gsl::HIST_ROWS);
  hipLaunchKernelGGL(gsl::k_map_age_hist, dim3(hist_blocks), dim3(gsl::HIST_THREADS), 0, st, stamps, (long long)n_rows,
                     now, w.bins);
  GSL_CHECK_LAUNCH();
  hipLaunchKernelGGL(gsl::k_map_age_threshold, dim3(1), dim3(gsl::HIST_THREADS), 0, st, w.bins, min_age,
                     (long long)need, w.params);
  GSL_CHECK_LAUNCH();
  hipLaunchKernelGGL(gsl::k_map_age_ties, dim3(nb), dim3(gsl::COMPACT_THREADS), 0, st, stamps, (long long)n_rows, now,
                     w.params, w.tie_ballots, tie_counts);
  GSL_CHECK_LAUNCH();
  gsl::launch_count_scan(st, tie_counts, nb, tie_bases, (int32_t*)(w.params + 3));
  GSL_CHECK_LAUNCH();
  hipLaunchKernelGGL(gsl::k_map_evict_select, dim3(nb), dim3(gsl::COMPACT_THREADS), 0, st, stamps, (long long)n_rows,
                     now, w.params, w.tie_ballots, tie_bases, w.head.ballots, w.head.counts, counters);
  GSL_CHECK_LAUNCH();
  gsl::launch_count_scan(st, w.head.counts, nb, w.head.bases, counters);
  GSL_CHECK_LAUNCH();
  return GSL_OK;
}

extern "C" int gsl_map_gather_i32(const int32_t* src, int64_t n_src, const int32_t* ids, int64_t n_ids, int32_t* dst,
                                  void* stream) {
  if (!src || !ids || !dst) return GSL_ERR_BAD_ARG;
  if (!gsl::map_rows_ok(n_src) || n_ids < 0 || n_ids >= 0x80000000ll) return GSL_ERR_BAD_ARG;
  if (n_ids == 0) return GSL_OK;
  hipLaunchKernelGGL(gsl::k_map_gather_i32, dim3((unsigned)((n_ids + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                     src, (long long)n_src, ids, (long long)n_ids, dst);
  GSL_CHECK_LAUNCH();
  return GSL_OK;
}
