// Long tile lists split over workgroups: segment sizes and the views into the caller's long_ws (tile_sort.hip: sort;
// raster_px.hip: k_long_map and the forward; raster_g16.hip: backward).
#pragma once
#include "gsloc_common.h"

namespace gsl {

// GSL_SEG: entries per compositing segment (the walk of a segment is serial per pixel, so its length is the latency of
// a pile frame: 512 -> 256 -> 128 took the pile frame's compositing from 0.50 to 0.37 to ... ms); GSL_SORT_SEG: keys per
// sorted run of the long-list sort (a multiple of GSL_SEG: 8 keys per lane in registers).
#ifndef GSL_SEG_LOG2
#define GSL_SEG_LOG2 7
#endif
#define GSL_SEG (1 << GSL_SEG_LOG2)
#define GSL_SORT_SEG_LOG2 9
#define GSL_SORT_SEG (1 << GSL_SORT_SEG_LOG2)

struct LongWs {  // views into the caller's long_ws (sized by gsl_long_ws_bytes)
  int32_t* n_seg;     // [4]: segments of this frame, max_seg overflow flag, -, -
  int32_t* seg_tile;  // [max_seg]
  int32_t* seg_idx;   // [max_seg]  segment number inside its tile
  int32_t* seg_cnt;   // [max_seg]  segments of that tile
  int32_t* seg_qcnt;  // [max_seg][4] length of the segment's hit list per quadrant (written by the forward's pass B)
  float* P;           // [max_seg][256]
  float* Tend;        // [max_seg][256]
  int32_t* last;      // [max_seg][256]
  float* C;           // [max_seg][256][4]
};
__host__ __device__ __forceinline__ LongWs long_ws_views(void* ws, int max_seg) {
  LongWs w;
  char* p = (char*)ws;
  w.n_seg = (int32_t*)p; p += 16;
  w.seg_tile = (int32_t*)p; p += (size_t)max_seg * 4;
  w.seg_idx = (int32_t*)p; p += (size_t)max_seg * 4;
  w.seg_cnt = (int32_t*)p; p += (size_t)max_seg * 4;
  w.seg_qcnt = (int32_t*)p; p += (size_t)max_seg * 16;
  p = (char*)(((uintptr_t)p + 255) & ~(uintptr_t)255);
  w.P = (float*)p; p += (size_t)max_seg * 256 * 4;
  w.Tend = (float*)p; p += (size_t)max_seg * 256 * 4;
  w.last = (int32_t*)p; p += (size_t)max_seg * 256 * 4;
  w.C = (float*)p;
  return w;
}

}  // namespace gsl
