// Frame-to-map localisation, the row rule, the one copy: where a row of the map lies in a frame.  Used by the view
// selection (map_view.hip), free space (map_free.hip), the observation stamps (map_evict.hip), the pose scores
// (map_score.hip), the refinement (map_refine.hip, which takes z, u, v and leaves the rounded uf, vf alone) and the pose
// information (map_info.hip, which takes the camera x and y as well); what each of them does with the projected row --
// its depth predicates, its counts -- is in its file.  The trajectory correction (map_correct.hip) projects nothing: it
// takes the row load and its store twin, and writes the bracket order of the rule out once more for its 3 x 4 entries.
//
// Row i of means[n,3], with w the rows of w2c (world to camera, row-major):
//   x = ((w0 px + w1 py) + w2 pz) + w3, y and z likewise;  u = fx x / z + cx, v = fy y / z + cy;
//   uf = rintf(u), vf = rintf(v) (round half to even: depth_to_points puts pixel u at (u - cx) / fx, a pixel's own
//   point projects onto the integer u);
//   in the band = z > near and z < far and lo <= u <= u_hi and lo <= v <= v_hi -- the image widened by a guard band of
//                 -lo pixels; the two upper limits, (width - 1) + guard and (height - 1) + guard, are float32 sums
//                 taken on the host;
//   inside      = 0 <= uf <= width - 1 and 0 <= vf <= height - 1 (float comparisons, then the conversion;
//                 rintf(-0.5) = -0 passes and is column 0);
//   the window  = the pixels (uf + du, vf + dv), |du|, |dv| <= window <= MAP_MAX_WINDOW, that are INSIDE the image.
// float32, every operation rounded once in the order written (no contraction, correctly rounded division), comparisons
// that are false for a NaN: on given inputs the rule has no rounding freedom, and the numpy mirrors of the tests
// (tests/map_*_ref.py, each with its own copy on purpose) decide identically.
// The 12-byte rows do not line up with lanes: a lane reads its row with one global_load_dwordx3, a wave's 768 contiguous
// bytes are six 128-byte lines that this one instruction touches once each ("Map growth": what the ISA
// shows and why the rows do not go through LDS).
// The argument checks that the map's entry points share are here too, as compact_ws_bytes is in compact_dev.h.
#pragma once
#include <math.h>

#include "gsloc_common.h"

namespace gsl {

constexpr int MAP_MAX_WINDOW = 3;  // window_px is 0 .. MAP_MAX_WINDOW (the entry points refuse anything else)

// What an entry point refuses with GSL_ERR_BAD_ARG when one of these is false: counts and indices are 32-bit.
static inline bool map_rows_ok(int64_t n_rows) { return n_rows > 0 && n_rows < 0x80000000ll; }
static inline bool map_image_ok(int width, int height) {
  return width > 0 && height > 0 && (long long)width * height <= 0x7fffffffll;
}
static inline bool map_focal_ok(float fx, float fy) { return fx != 0.f && fy != 0.f; }

struct MapPixel {  // a projected row: its depth, its image position, the position rounded to a pixel
  float z, u, v, uf, vf;
};
struct MapWindow {  // u0 .. u1 x v0 .. v1, inclusive
  int u0, u1, v0, v1;
};

__device__ static inline float3 map_load_row(const float* __restrict__ means, long long g) {
  return {means[3 * (size_t)g], means[3 * (size_t)g + 1], means[3 * (size_t)g + 2]};
}

// The store twin: a lane writes its own row with one global_store_dwordx3.
__device__ static inline void map_store_row(float* __restrict__ means, long long g, float3 r) {
  means[3 * (size_t)g] = r.x;
  means[3 * (size_t)g + 1] = r.y;
  means[3 * (size_t)g + 2] = r.z;
}

// w: the twelve leading entries of a row-major world-to-camera matrix.  cam_x, cam_y: the row's camera x and y, which
// the pixel is made from (its camera z is MapPixel::z) -- for the caller that needs the point itself (map_info.hip).
__device__ static inline MapPixel map_project_point(const float* __restrict__ w, float3 r, float fx, float fy, float cx,
                                                    float cy, float& cam_x, float& cam_y) {
#pragma clang fp contract(off)
  const float x = ((w[0] * r.x + w[1] * r.y) + w[2] * r.z) + w[3];
  const float y = ((w[4] * r.x + w[5] * r.y) + w[6] * r.z) + w[7];
  const float z = ((w[8] * r.x + w[9] * r.y) + w[10] * r.z) + w[11];
  const float u = fx * x / z + cx, v = fy * y / z + cy;
  cam_x = x;
  cam_y = y;
  return {z, u, v, rintf(u), rintf(v)};
}

__device__ static inline MapPixel map_project(const float* __restrict__ w, float3 r, float fx, float fy, float cx,
                                              float cy) {
  float x, y;
  return map_project_point(w, r, fx, fy, cx, cy, x, y);
}

// (p by value: behind a reference the chain's short circuits guard loads, and k_map_view_select keeps a branch for them)
__device__ static inline bool map_in_band(MapPixel p, float near_plane, float far_plane, float lo, float u_hi,
                                          float v_hi) {
  return p.z > near_plane && p.z < far_plane && p.u >= lo && p.u <= u_hi && p.v >= lo && p.v <= v_hi;
}

// u_last, v_last: (float)(width - 1), (float)(height - 1).  True: uf, vf are integers in [0, width - 1] x
// [0, height - 1], and every index of map_window is inside the image.
__device__ static inline bool map_inside(const MapPixel& p, float u_last, float v_last) {
  return p.uf >= 0.f && p.uf <= u_last && p.vf >= 0.f && p.vf <= v_last;
}

// For a row that is map_inside.
__device__ static inline MapWindow map_window(const MapPixel& p, int window, int width, int height) {
  const int uc = (int)p.uf, vc = (int)p.vf;
  return {uc - window > 0 ? uc - window : 0, uc + window < width - 1 ? uc + window : width - 1,
          vc - window > 0 ? vc - window : 0, vc + window < height - 1 ? vc + window : height - 1};
}

}  // namespace gsl
