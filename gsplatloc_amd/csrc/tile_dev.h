// Shared by the binning kernels (binning.hip, fused_project.hip) and the deterministic row gather of the projection
// backward (fused_project_bwd.hip).
#pragma once
#include "gsloc_common.h"

namespace gsl {

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

}  // namespace gsl
