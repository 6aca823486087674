// Shared by the binning kernels (binning.hip, fused_project.hip) and the deterministic row gather of the projection
// backward (fused_project_bwd.hip).
#pragma once
#include "gsloc_common.h"

namespace gsl {

// The kernels that keep one LDS counter per tile of the strip (the projection's histogram, the count and the scatter of
// two-pass binning): threads per workgroup, and the most tiles a strip may have for them.
#ifndef GSL_BIN_THREADS
#define GSL_BIN_THREADS 512
#endif
#define GSL_MAX_STRIP_TILES 8192

// Tile rectangle of a projected Gaussian: [xmin,xmax) x [ymin,ymax) in tiles.
__device__ __forceinline__ void tile_rect(float mx, float my, int radius, int tile_size, int tile_w,
                                          int tile_h, int& xmin, int& ymin, int& xmax, int& ymax) {
  float ts = (float)tile_size;
  float tr = (float)radius / ts;
  float tx = mx / ts, ty = my / ts;
  // clamp in float first: (uint32_t)floor(negative) saturates to 0 in the reference kernel
  xmin = (int)fminf(fmaxf(floorf(tx - tr), 0.f), (float)tile_w);
  ymin = (int)fminf(fmaxf(floorf(ty - tr), 0.f), (float)tile_h);
  xmax = (int)fminf(fmaxf(ceilf(tx + tr), 0.f), (float)tile_w);
  ymax = (int)fminf(fmaxf(ceilf(ty + tr), 0.f), (float)tile_h);
}

// The same, clipped to the strip of tile rows [ty0, ty1): empty (ymax == ymin) when the rectangle misses the strip.
__device__ __forceinline__ void strip_rect(float mx, float my, int radius, int tile_size, int tile_w, int tile_h, int ty0,
                                           int ty1, int& xmin, int& ymin, int& xmax, int& ymax) {
  tile_rect(mx, my, radius, tile_size, tile_w, tile_h, xmin, ymin, xmax, ymax);
  ymin = max(ymin, ty0);
  ymax = min(ymax, ty1);
  if (ymax < ymin) ymax = ymin;
}

}  // namespace gsl
