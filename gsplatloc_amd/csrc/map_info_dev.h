// Frame-to-map localisation, the normal equations of a pose, the one copy: what a workgroup of k_map_pose_info
// (map_info.hip, where the rule and its bounds are written down) does with its rows -- the per-row arithmetic, the sums
// in registers, the wave and LDS reduction and the integer atomics on out.  k_map_pose_info is this function for one
// pose; the batched alignment (map_align_batch.hip) calls it with the pose and the sums of blockIdx.y.  The workgroups
// of a pose are those along blockIdx.x either way; how many there are, and of how many threads, is the caller's grid.
// PHOTO adds the photometric equation of a used row (map_photo.hip, where that rule and its bound are written down) into
// the same sums; without it the colour arguments are not read and the function is what it was before they existed.
#pragma once
#include "gsloc_common.h"
#include "map_dev.h"

namespace gsl {

constexpr int INFO_SUMS = 28;          // 21 + 6 + 1 fixed-point sums; then the two counts
constexpr float INFO_MAX_DEPTH = 64.f;
constexpr float INFO_ONE = 1048576.f;  // 2^20
constexpr float INFO_PHOTO_MAX_A = 8.f;       // |a_k| of a photometric equation (map_photo.hip: the bound)
constexpr float INFO_PHOTO_MAX_DEPTH = 16.f;  // z of a row that gives one
constexpr float INFO_PHOTO_MAX_SCALE = 16.f;  // photo_scale, metres per unit of intensity
static_assert(INFO_SUMS + 2 == GSL_MAP_INFO_VALUES, "out is the sums and the two counts");

// Where fix(J_a, J_b), a <= b <= 6 with J_6 = r, goes in out.
__host__ __device__ constexpr int info_slot(int a, int b) {
  return b < 6 ? a * 6 - a * (a - 1) / 2 + (b - a) : a < 6 ? 21 + a : 27;
}
static_assert(info_slot(0, 0) == 0 && info_slot(0, 5) == 5 && info_slot(1, 1) == 6 && info_slot(5, 5) == 20 &&
                  info_slot(0, 6) == 21 && info_slot(5, 6) == 26 && info_slot(6, 6) == 27,
              "the upper triangle row-major, then g, then the residual sum");

__device__ static inline long long info_fix(float s, float t) {
#pragma clang fp contract(off)
  return llrintf((s * t) * INFO_ONE);
}

__device__ static inline bool info_neighbour_ok(float d, float lo, float hi) {
  return d > 0.f && d < INFINITY && d >= lo && d <= hi;
}

__device__ static inline bool info_in01(float t) { return t >= 0.f && t <= 1.f; }

// The photometric arguments of an entry point, as the launch sequences hand them on: the rows' colours, the frame's
// intensity image, photo_scale and photo_max_residual.  A sequence that is given none (NULL) sums geometry alone.
struct InfoPhoto {
  const float* colors;
  const float* intensity;
  float scale, max_residual;
};

// What the photometric entry points refuse alike before any launch, beside what their geometric twins refuse.
static inline bool info_photo_args_ok(const InfoPhoto& p) {
  return p.colors && p.intensity && p.scale >= 0.f && p.scale <= INFO_PHOTO_MAX_SCALE && p.max_residual >= 0.f &&
         p.max_residual <= 1.f;
}

// Every thread of a workgroup of THREADS calls this (it holds barriers); the rows are strided by gridDim.x.
// PHOTO: colors[n,3] the rows' colours, intensity[height,width] the frame's (map_photo.hip), s = photo_scale,
// photo_max = photo_max_residual, extra NULL or int64[2] (rows with a photometric equation, the sum of their
// fix(s rc, s rc)); none of them is touched without it.
template <int THREADS, bool PHOTO>
__device__ static inline void info_sum_rows(const float* __restrict__ means, long long n_rows,
                                            const float* __restrict__ w2c, float fx, float fy, float cx, float cy,
                                            const float* __restrict__ depth, int width, float u_inner, float v_inner,
                                            float keep, float beyond, float kappa, float near_plane,
                                            unsigned long long* __restrict__ out, const float* __restrict__ colors,
                                            const float* __restrict__ intensity, float s, float photo_max,
                                            unsigned long long* __restrict__ extra) {
  constexpr int TABLE = GSL_MAP_INFO_VALUES + (PHOTO ? 2 : 0);
  static_assert(TABLE <= THREADS, "one thread per entry of the table flushes it");
  __shared__ unsigned long long table[TABLE];
  if ((int)threadIdx.x < TABLE) table[threadIdx.x] = 0ull;
  __syncthreads();
  long long acc[INFO_SUMS];
#pragma unroll
  for (int i = 0; i < INFO_SUMS; ++i) acc[i] = 0;
  long long acc_photo = 0;                 // PHOTO: the colour share of slot 27
  uint32_t n_used = 0u, n_tested = 0u;     // the wave's: wave-uniform
  uint32_t n_photo = 0u;
  const long long stride = (long long)gridDim.x * THREADS;
  // the trip count is the workgroup's: every lane of a wave reaches every ballot
  for (long long base = (long long)blockIdx.x * THREADS; base < n_rows; base += stride) {
#pragma clang fp contract(off)
    const long long g = base + threadIdx.x;
    const bool live = g < n_rows;
    float3 row = {0.f, 0.f, 0.f};
    if (live) row = map_load_row(means, g);
    float x, y;
    const MapPixel p = map_project_point(w2c, row, fx, fy, cx, cy, x, y);
    bool tested = live && p.z > near_plane && p.uf >= 1.f && p.uf <= u_inner && p.vf >= 1.f && p.vf <= v_inner;
    bool used = false;
    float J[7];
    size_t at = 0;
    if (tested) {  // the five indices are inside
      at = (size_t)(int)p.vf * (size_t)width + (size_t)(int)p.uf;
      const float d0 = depth[at];
      tested = d0 > 0.f && d0 < INFINITY;
      const float lo = d0 * keep, hi = d0 * beyond;
      if (tested && p.z >= lo && p.z <= hi && p.z < INFO_MAX_DEPTH) {
        const float dl = depth[at - 1], dr = depth[at + 1], du = depth[at - (size_t)width], dd = depth[at + (size_t)width];
        if (info_neighbour_ok(dl, lo, hi) && info_neighbour_ok(dr, lo, hi) && info_neighbour_ok(du, lo, hi) &&
            info_neighbour_ok(dd, lo, hi)) {
          const float i0 = 1.f / d0, s0 = i0 + i0, tol = kappa * i0;
          const float su = 1.f / dl + 1.f / dr, sv = 1.f / du + 1.f / dd;
          if (fabsf(su - s0) <= tol && fabsf(sv - s0) <= tol) {
            // q(u, v, d): the back-projection of k_map_append
            const float kx0 = (p.uf - cx) / fx, ky0 = (p.vf - cy) / fy;
            const float kxl = ((p.uf - 1.f) - cx) / fx, kxr = ((p.uf + 1.f) - cx) / fx;
            const float kyu = ((p.vf - 1.f) - cy) / fy, kyd = ((p.vf + 1.f) - cy) / fy;
            const float ax = kxr * dr - kxl * dl, ay = ky0 * dr - ky0 * dl, az = dr - dl;
            const float bx = kx0 * dd - kx0 * du, by = kyd * dd - kyu * du, bz = dd - du;
            const float c0 = ay * bz - az * by, c1 = az * bx - ax * bz, c2 = ax * by - ay * bx;
            const float len = sqrtf((c0 * c0 + c1 * c1) + c2 * c2);
            if (len > 0.f) {
              const float n0 = c0 / len, n1 = c1 / len, n2 = c2 / len;
              const float e0 = x - kx0 * d0, e1 = y - ky0 * d0, e2 = p.z - d0;
              J[0] = y * n2 - p.z * n1;
              J[1] = p.z * n0 - x * n2;
              J[2] = x * n1 - y * n0;
              J[3] = n0;
              J[4] = n1;
              J[5] = n2;
              J[6] = (n0 * e0 + n1 * e1) + n2 * e2;
              used = true;
            }
          }
        }
      }
    }
    if (used) {
#pragma unroll
      for (int a = 0; a < 7; ++a)
#pragma unroll
        for (int b = a; b < 7; ++b) acc[info_slot(a, b)] += info_fix(J[a], J[b]);
    }
    n_tested += (uint32_t)__popcll(__ballot(tested));
    n_used += (uint32_t)__popcll(__ballot(used));
    if constexpr (PHOTO) {
      bool photo = false;
      if (used) {  // at is an inner pixel: the five indices are inside
        const float3 c = map_load_row(colors, g);
        const float Yi = (0.299f * c.x + 0.587f * c.y) + 0.114f * c.z;
        const float Y0 = intensity[at], Yl = intensity[at - 1], Yr = intensity[at + 1];
        const float Yu = intensity[at - (size_t)width], Yd = intensity[at + (size_t)width];
        if (info_in01(Yi) && info_in01(Y0) && info_in01(Yl) && info_in01(Yr) && info_in01(Yu) && info_in01(Yd)) {
          const float gx = (Yr - Yl) * 0.5f, gy = (Yd - Yu) * 0.5f;
          const float Yp = (Y0 + gx * (p.u - p.uf)) + gy * (p.v - p.vf);
          const float rc = Yp - Yi;
          if (fabsf(rc) <= photo_max) {
            const float a0 = (s * gx) * fx / p.z, a1 = (s * gy) * fy / p.z;
            const float a2 = -((a0 * x + a1 * y) / p.z);
            if (fabsf(a0) <= INFO_PHOTO_MAX_A && fabsf(a1) <= INFO_PHOTO_MAX_A && fabsf(a2) <= INFO_PHOTO_MAX_A &&
                p.z < INFO_PHOTO_MAX_DEPTH) {
              J[0] = y * a2 - p.z * a1;
              J[1] = p.z * a0 - x * a2;
              J[2] = x * a1 - y * a0;
              J[3] = a0;
              J[4] = a1;
              J[5] = a2;
              J[6] = s * rc;
              photo = true;
            }
          }
        }
      }
      if (photo) {
#pragma unroll
        for (int a = 0; a < 7; ++a)
#pragma unroll
          for (int b = a; b < 7; ++b) {
            const long long t = info_fix(J[a], J[b]);
            acc[info_slot(a, b)] += t;
            if (a == 6) acc_photo += t;
          }
      }
      n_photo += (uint32_t)__popcll(__ballot(photo));
    }
  }
  // per wave, then LDS
  const bool first_lane = (threadIdx.x & 63) == 0;
#pragma unroll
  for (int i = 0; i < INFO_SUMS; ++i) {
    long long v = acc[i];
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off);
    if (first_lane && v != 0) atomicAdd(&table[i], (unsigned long long)v);
  }
  if (first_lane && n_tested != 0u) {
    atomicAdd(&table[INFO_SUMS + 1], (unsigned long long)n_tested);
    if (n_used != 0u) atomicAdd(&table[INFO_SUMS], (unsigned long long)n_used);
  }
  if constexpr (PHOTO) {
    long long v = acc_photo;
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off);
    if (first_lane && n_photo != 0u) {
      atomicAdd(&table[GSL_MAP_INFO_VALUES], (unsigned long long)n_photo);
      if (v != 0) atomicAdd(&table[GSL_MAP_INFO_VALUES + 1], (unsigned long long)v);
    }
  }
  __syncthreads();
  if ((int)threadIdx.x < GSL_MAP_INFO_VALUES) {
    const unsigned long long c = table[threadIdx.x];
    if (c != 0ull) atomicAdd(&out[threadIdx.x], c);
  }
  if constexpr (PHOTO) {
    if (extra && (int)threadIdx.x >= GSL_MAP_INFO_VALUES && (int)threadIdx.x < TABLE) {
      const unsigned long long c = table[threadIdx.x];
      if (c != 0ull) atomicAdd(&extra[threadIdx.x - GSL_MAP_INFO_VALUES], c);
    }
  }
}

}  // namespace gsl
