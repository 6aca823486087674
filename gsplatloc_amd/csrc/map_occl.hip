// Frame-to-map localisation: occlusion culling of the local map.  The view selection (map_view.hip) takes every row
// inside the frustum; here a row that lies behind a nearer surface of the map itself is left out as well
// (gsplatloc_amd/mapping.py: select_view(occlusion_rho=), view_violations, view_depth).
//
// The grid.  gi = (int)ceilf(guard_px); cells of cell_px x cell_px pixels (1, 2, 4, 8 or 16) over the image widened by gi:
//   CW = (width - 1 + 2 gi) / cell_px + 1, CH likewise (integer division).  A row in the band (map_dev.h, lo = -guard_px,
//   as k_map_view_select evaluates it) lies in the cell
//   cu = (int)floorf((u + (float)gi) * inv_cell), cv = (int)floorf((v + (float)gi) * inv_cell), inv_cell = 1 / cell_px, a
//   power of two: the product is exact.  0 <= cu < CW and 0 <= cv < CH without a clamp: u >= -guard_px >= -gi, and
//   u <= fl((width - 1) + guard_px) <= (width - 1) + gi, an integer that float32 holds exactly -- the entry points refuse
//   a grid whose widened image is not below 2^24 pixels a side -- so fl(u + gi) <= (width - 1) + 2 gi.
// Pass 1, k_map_occl_depth: zbuf[CH CW] uint32, cleared to 0 (zero_u32, never a memset node: misc.hip); every row in the
//   band does atomicMax(zbuf[cv CW + cu], ~bits(z)).  near_plane >= 0, so z > 0: its bit pattern orders as the float does
//   and the complement turns the maximum into the NEAREST depth; 0 is "no row here", which no row in the band produces.
//   Integer atomics: the buffer does not depend on the order of rows, waves or workgroups.
// Pass 2, k_map_occl_select: m = the minimum of zbuf over the cells (cu + du, cv + dv), |du|, |dv| <= window, a cell
//   outside the grid counting as 0; the row is OCCLUDED when m != 0 and keep * z > asfloat(~m) (one rounded product,
//   keep = 1 - rho taken by the caller); SELECTED = in the band and not occluded.  A row goes only when every cell around
//   it holds a surface nearer than (1 - rho) z: an empty cell, the silhouette of an occluder and a lone ghost row keep it.
//   The ballots, counts and bases are those of k_map_view_select (compact_dev.h), so gsl_map_view_gather follows
//   unchanged; a third mask -- in the band and occluded -- is counted and scanned into counters[3].
// float32, every operation rounded once in the order written, comparisons false for a NaN: the numpy mirror
// (tests/map_occl_ref.py) decides identically.
//
// Pass 1 is the hot kernel: one row per thread, one global_load_dwordx3, and then the hazard -- the rows of a frame sit
// in the map in raster order, so neighbouring lanes fall into the same cell and naive atomics pile up on a few words
// (k_map_covis: 56 us against 8).  Two remedies, both built (the template arguments; scripts/occl_cost.py measures a
// library made with -DGSL_OCCL_PRELOAD= / -DGSL_OCCL_COMBINE=).  At 460 800 rows in raster order the kernel takes
// 27.0 us with neither, 20.8 with PRELOAD, 4.0 with COMBINE and 4.4 with both; on rows in random order, where no two
// neighbouring lanes share a cell, 21.8 / 51.4 / 22.4 / 55.5 -- the load in front of the atomic is a dependent round
// trip to a line the atomics keep out of L2.  COMBINE alone is what the library is built with:
//   COMBINE  a segmented maximum over the wave's runs of equal cell: four row_shr steps inside a DPP row of 16 lanes,
//            row_bcast15 and row_bcast31 across the rows; a lane adopts another lane's key whenever that lane's cell is
//            its own, run or not -- the maximum of a cell is wanted, so that is never wrong.  The last lane of each run
//            (wave_shl:1 shows the next lane's cell) then holds the run's maximum and issues the one atomic.
//   PRELOAD  the issuing lane first reads the cell with a plain load and skips the atomic when the stored key is already
//            >= its own.  Keys only grow: a stale read costs a redundant atomic, never a wrong result.
#include "compact_dev.h"
#include "gsloc_internal.h"
#include "map_dev.h"

#ifndef GSL_OCCL_PRELOAD
#define GSL_OCCL_PRELOAD 0
#endif
#ifndef GSL_OCCL_COMBINE
#define GSL_OCCL_COMBINE 1
#endif

namespace gsl {

constexpr long long OCCL_MAX_CELLS = 1ll << 26;  // 256 MiB of keys
constexpr int OCCL_MAX_SIDE = 1 << 24;           // the widened image, pixels a side: float32 holds every integer below

struct OcclGrid {  // cw == 0: arguments the entry points refuse
  int gi, cw, ch;
};

// guard_px >= 0 (false for a NaN), cell_px one of 1, 2, 4, 8, 16.
static inline OcclGrid occl_grid(int width, int height, float guard_px, int cell_px) {
  const OcclGrid none = {0, 0, 0};
  if (!map_image_ok(width, height) || !(guard_px >= 0.f) || !(guard_px < (float)OCCL_MAX_SIDE)) return none;
  if (cell_px != 1 && cell_px != 2 && cell_px != 4 && cell_px != 8 && cell_px != 16) return none;
  const long long gi = (long long)ceilf(guard_px);
  const long long side_w = (long long)width - 1 + 2 * gi, side_h = (long long)height - 1 + 2 * gi;
  if (side_w >= OCCL_MAX_SIDE || side_h >= OCCL_MAX_SIDE) return none;
  const long long cw = side_w / cell_px + 1, ch = side_h / cell_px + 1;
  if (cw * ch > OCCL_MAX_CELLS) return none;
  return {(int)gi, (int)cw, (int)ch};
}

// The cell of a row that is in the band; gi_f = (float)gi.
__device__ static inline void occl_cell(const MapPixel& p, float gi_f, float inv_cell, int& cu, int& cv) {
#pragma clang fp contract(off)
  cu = (int)floorf((p.u + gi_f) * inv_cell);
  cv = (int)floorf((p.v + gi_f) * inv_cell);
}

// lane i <- lane i - n of its DPP row (row_shr:n), lane 15 of the row before (row_bcast15, rows 1 and 3), lane 31
// (row_bcast31, rows 2 and 3), lane i + 1 of the wave (wave_shl:1); a lane without a source keeps `old`.
template <int CTRL, int ROW_MASK = 0xF>
__device__ __forceinline__ int occl_dpp(int old, int v) {
  return __builtin_amdgcn_update_dpp(old, v, CTRL, ROW_MASK, 0xF, false);
}

// One step of the segmented maximum: the lanes that see a lane of their own cell take the larger key.  cell >= 0 in the
// lanes that take part, -1 elsewhere: no lane sees its own cell in `old`.
template <int CTRL, int ROW_MASK = 0xF>
__device__ __forceinline__ uint32_t occl_step(int cell, uint32_t key) {
  const int other_cell = occl_dpp<CTRL, ROW_MASK>(-2, cell);
  const uint32_t other_key = (uint32_t)occl_dpp<CTRL, ROW_MASK>(0, (int)key);
  return other_cell == cell && other_key > key ? other_key : key;
}

template <bool PRELOAD, bool COMBINE>
__global__ __launch_bounds__(COMPACT_THREADS) void k_map_occl_depth(
    const float* __restrict__ means, long long n_rows, const float* __restrict__ w2c, float fx, float fy, float cx,
    float cy, float guard_lo, float u_hi, float v_hi, float near_plane, float far_plane, float gi_f, float inv_cell,
    int cw, int ch, uint32_t* zbuf) {
  const long long g = (long long)blockIdx.x * COMPACT_THREADS + threadIdx.x;
  int cell = -1;
  uint32_t key = 0u;
  if (g < n_rows) {
    const MapPixel p = map_project(w2c, map_load_row(means, g), fx, fy, cx, cy);
    if (map_in_band(p, near_plane, far_plane, guard_lo, u_hi, v_hi)) {
      int cu, cv;
      occl_cell(p, gi_f, inv_cell, cu, cv);
      // the grid holds the band (above); the comparison keeps a write inside zbuf whatever the arithmetic did
      if ((unsigned)cu < (unsigned)cw && (unsigned)cv < (unsigned)ch) {
        cell = cv * cw + cu;
        key = ~__float_as_uint(p.z);
      }
    }
  }
  bool issue = cell >= 0;
  if (COMBINE) {  // every lane of the wave is here: the exchanges read lanes without a row as cell -1
    key = occl_step<0x111>(cell, key);        // row_shr:1
    key = occl_step<0x112>(cell, key);        // row_shr:2
    key = occl_step<0x114>(cell, key);        // row_shr:4
    key = occl_step<0x118>(cell, key);        // row_shr:8
    key = occl_step<0x142, 0xA>(cell, key);   // row_bcast15 into rows 1 and 3
    key = occl_step<0x143, 0xC>(cell, key);   // row_bcast31 into rows 2 and 3
    issue = issue && occl_dpp<0x130>(-2, cell) != cell;  // wave_shl:1: the next lane is in another cell, or there is none
  }
  if (!issue) return;
  if (PRELOAD && zbuf[cell] >= key) return;
  atomicMax(&zbuf[cell], key);
}

__global__ __launch_bounds__(COMPACT_THREADS) void k_map_occl_select(
    const float* __restrict__ means, long long n_rows, const float* __restrict__ w2c, float fx, float fy, float cx,
    float cy, float guard_lo, float u_hi, float v_hi, float near_plane, float far_plane, float gi_f, float inv_cell,
    int cw, int ch, int window, float keep, const uint32_t* __restrict__ zbuf,
    const uint64_t* __restrict__ prev_ballots, uint64_t* __restrict__ ballots, uint32_t* __restrict__ block_counts,
    uint32_t* __restrict__ block_fresh, uint32_t* __restrict__ block_culled, int32_t* __restrict__ counters) {
#pragma clang fp contract(off)
  const long long g = (long long)blockIdx.x * COMPACT_THREADS + threadIdx.x;
  if (g == 0) {  // the scans that follow in the stream write [0], [3] and, with prev, [1]
    if (prev_ballots == nullptr) counters[1] = 0;
    counters[2] = 0;  // nothing gathered yet
  }
  bool in_band = false, occluded = false;
  if (g < n_rows) {
    const MapPixel p = map_project(w2c, map_load_row(means, g), fx, fy, cx, cy);
    in_band = map_in_band(p, near_plane, far_plane, guard_lo, u_hi, v_hi);
    if (in_band) {
      int cu, cv;
      occl_cell(p, gi_f, inv_cell, cu, cv);
      uint32_t m = 0xffffffffu;
      for (int dv = -window; dv <= window; ++dv)
        for (int du = -window; du <= window; ++du) {
          const int a = cu + du, b = cv + dv;
          const bool inside = (unsigned)a < (unsigned)cw && (unsigned)b < (unsigned)ch;
          const uint32_t k = inside ? zbuf[(size_t)b * (size_t)cw + (size_t)a] : 0u;
          m = k < m ? k : m;
        }
      occluded = m != 0u && keep * p.z > __uint_as_float(~m);
    }
  }
  const unsigned long long sel = compact_ballot(in_band && !occluded, ballots);
  // second mask: selected now, bit clear in prev; third: in the band and occluded
  const unsigned long long mask[3] = {sel, prev_ballots ? sel & ~prev_ballots[compact_wave_slot()] : 0ull,
                                      __ballot(in_band && occluded)};
  uint32_t sum[3];
  if (compact_block_sums(mask, sum)) {
    block_counts[blockIdx.x] = sum[0];
    if (prev_ballots) block_fresh[blockIdx.x] = sum[1];
    block_culled[blockIdx.x] = sum[2];
  }
}

}  // namespace gsl

extern "C" size_t gsl_map_occl_zbuf_bytes(int width, int height, float guard_px, int cell_px) {
  const gsl::OcclGrid grid = gsl::occl_grid(width, height, guard_px, cell_px);
  return (size_t)grid.cw * (size_t)grid.ch * sizeof(uint32_t);
}

extern "C" size_t gsl_map_occl_ws_bytes(int64_t n_rows) {
  // four extra columns: the second counts and their bases (where gsl_map_view_select has them), the occluded counts and
  // their bases
  return gsl::compact_ws_bytes(n_rows < 0x80000000ll ? (long long)n_rows : 0, 4);
}

// Argument checks shared by the two passes; the grid on success.
static int occl_check(const float* means, int64_t n_rows, const float* w2c, float fx, float fy, int width, int height,
                      float guard_px, int cell_px, float near_plane, float far_plane, const void* zbuf,
                      size_t zbuf_bytes, gsl::OcclGrid& grid) {
  if (!means || !w2c || !zbuf) return GSL_ERR_BAD_ARG;
  if (!gsl::map_rows_ok(n_rows) || !gsl::map_image_ok(width, height) || !gsl::map_focal_ok(fx, fy)) return GSL_ERR_BAD_ARG;
  if (!(guard_px >= 0.f) || !(near_plane >= 0.f) || !(near_plane < far_plane)) return GSL_ERR_BAD_ARG;
  grid = gsl::occl_grid(width, height, guard_px, cell_px);
  if (grid.cw == 0) return GSL_ERR_BAD_ARG;
  if (zbuf_bytes < (size_t)grid.cw * (size_t)grid.ch * sizeof(uint32_t)) return GSL_ERR_WORKSPACE;
  return GSL_OK;
}

extern "C" int gsl_map_occl_depth(const float* means, int64_t n_rows, const float* w2c, float fx, float fy, float cx,
                                  float cy, int width, int height, float guard_px, int cell_px, float near_plane,
                                  float far_plane, void* zbuf, size_t zbuf_bytes, void* stream) {
  gsl::OcclGrid grid;
  int rc = occl_check(means, n_rows, w2c, fx, fy, width, height, guard_px, cell_px, near_plane, far_plane, zbuf,
                      zbuf_bytes, grid);
  if (rc != GSL_OK) return rc;
  hipStream_t st = (hipStream_t)stream;
  rc = gsl::zero_u32(zbuf, (size_t)grid.cw * (size_t)grid.ch, st);
  if (rc != GSL_OK) return rc;
  const int nb = (int)gsl::compact_blocks(n_rows);
  const float u_hi = (float)(width - 1) + guard_px, v_hi = (float)(height - 1) + guard_px;  // one float32 sum each
  hipLaunchKernelGGL((gsl::k_map_occl_depth<GSL_OCCL_PRELOAD != 0, GSL_OCCL_COMBINE != 0>), dim3(nb),
                     dim3(gsl::COMPACT_THREADS), 0, st, means, (long long)n_rows, w2c, fx, fy, cx, cy, -guard_px, u_hi,
                     v_hi, near_plane, far_plane, (float)grid.gi, 1.f / (float)cell_px, grid.cw, grid.ch,
                     (uint32_t*)zbuf);
  GSL_CHECK_LAUNCH();
  return GSL_OK;
}

extern "C" int gsl_map_occl_select(const float* means, int64_t n_rows, const float* w2c, float fx, float fy, float cx,
                                   float cy, int width, int height, float guard_px, float near_plane, float far_plane,
                                   int cell_px, int window, float rho_keep, const void* zbuf, size_t zbuf_bytes,
                                   const void* prev_ws, int32_t* counters, void* ws, size_t ws_bytes, void* stream) {
  gsl::OcclGrid grid;
  int rc = occl_check(means, n_rows, w2c, fx, fy, width, height, guard_px, cell_px, near_plane, far_plane, zbuf,
                      zbuf_bytes, grid);
  if (rc == GSL_ERR_BAD_ARG) return rc;
  if (!counters || !ws || (prev_ws != nullptr && prev_ws == ws)) return GSL_ERR_BAD_ARG;
  if (window < 0 || window > gsl::MAP_MAX_WINDOW || !(rho_keep > 0.f && rho_keep < 1.f)) return GSL_ERR_BAD_ARG;
  if (rc != GSL_OK) return rc;
  if (ws_bytes < gsl_map_occl_ws_bytes(n_rows)) return GSL_ERR_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  const int nb = (int)gsl::compact_blocks(n_rows);
  const gsl::CompactWs w = gsl::compact_ws(ws, nb);
  uint32_t *fresh = w.extra, *fresh_bases = w.extra + nb, *culled = w.extra + 2 * (size_t)nb,
           *culled_bases = w.extra + 3 * (size_t)nb;
  const float u_hi = (float)(width - 1) + guard_px, v_hi = (float)(height - 1) + guard_px;  // one float32 sum each
  hipLaunchKernelGGL(gsl::k_map_occl_select, dim3(nb), dim3(gsl::COMPACT_THREADS), 0, st, means, (long long)n_rows, w2c,
                     fx, fy, cx, cy, -guard_px, u_hi, v_hi, near_plane, far_plane, (float)grid.gi,
                     1.f / (float)cell_px, grid.cw, grid.ch, window, rho_keep, (const uint32_t*)zbuf,
                     (const uint64_t*)prev_ws, w.ballots, w.counts, fresh, culled, counters);
  GSL_CHECK_LAUNCH();
  gsl::launch_count_scan(st, w.counts, nb, w.bases, counters);
  GSL_CHECK_LAUNCH();
  if (prev_ws) {
    gsl::launch_count_scan(st, fresh, nb, fresh_bases, counters + 1);
    GSL_CHECK_LAUNCH();
  }
  gsl::launch_count_scan(st, culled, nb, culled_bases, counters + 3);
  GSL_CHECK_LAUNCH();
  return GSL_OK;
}
