// Frame-to-map localisation: exposure compensation for the photometric term (gsplatloc_amd/mapping.py:
// GaussianMap.estimate_exposure, apply_exposure; MapConfig.photo_exposure).  The photometric equation (map_photo.hip)
// holds a row's stored colour against the frame's intensity as if every frame had the exposure of the map's first one.
// Here a frame gets an affine brightness model, gain * Y_frame + offset ~ Y_row over the rows of the map that the frame
// sees: two parameters, estimated by least squares on the device and applied to the frame's rgb once.  The intensity
// weights sum to one, Y(gain * rgb + 255 * offset) = gain * Y(rgb) + offset, so the corrected rgb has the corrected
// intensity, and everything downstream only ever receives a different image.
//
// k_map_exposure_sums.  Row i of means[n,3] with its colour c = colors[i], projected through w2c to z, uf, vf
// (map_dev.h: the one copy of the projection), float32, one rounding per operation in the order written, no
// contraction, comparisons false for a NaN:
//   seen = z > near and inside (0 <= uf <= width - 1, 0 <= vf <= height - 1) and d0 > 0 and d0 < inf,
//          d0 = depth[vf, uf], and d0 * keep <= z and z <= d0 * beyond -- the nearest pixel only: border pixels count;
//   Yi = (0.299f c.r + 0.587f c.g) + 0.114f c.b,  Y0 = intensity[vf, uf];
//   used = seen and sat_lo <= Yi <= sat_hi and sat_lo <= Y0 <= sat_hi (a clipped pixel follows no affine model)
//          and |(g0 * Y0 + b0) - Yi| <= gate, g0 = params[0], b0 = params[1] read from the device; gate is +inf in the
//          first pass (params = 1, 0) and max_residual afterwards: an occluder, a highlight or a wrong row is not exposure.
// With fix(s, t) = llrintf((s * t) * 2^20) (map_info_dev.h), out[7] int64 = sum fix(Y0, Y0), sum fix(Y0, 1),
// sum fix(Y0, Yi), sum fix(Yi, 1), sum fix(Yi, Yi), rows used, rows seen.  Integer sums do not depend on the order of
// rows, waves or workgroups, and tests/map_exposure_ref.py gives the same seven integers from numpy.
//
// No sum can overflow.  A used row has 0 <= sat_lo <= Y0, Yi <= sat_hi <= 1 (the entry point refuses another range): every
// product is in 0 .. 1, every term at most 2^20, and fewer than 2^31 rows (map_rows_ok) keep every sum below 2^51.
//
// One thread per row over a grid-stride loop, at most EXPOSURE_MAX_BLOCKS workgroups of 256 threads, as
// k_map_pose_info.  A lane keeps the five sums in ten registers over all its trips; the two counts are ballots and
// population counts in scalar registers.  After the rows each wave adds its lanes' sums (six xor-shuffle steps per
// value), lane 0 adds them to a table of 7 in LDS (56 B), and the workgroup adds its non-zero entries to out with one
// 64-bit integer atomic each.  No float atomics.  out is zeroed by a launch of zero_u32 in front (never a memset node).
//
// k_map_exposure_solve, pass k, one thread, float64, no contraction, one rounding per operation in the order written
// (the precedent: align_step of map_align_dev.h):
//   the seven integers are read; n = (double)used, Sxx, Sx, Sxy, Sy, Syy = (double)out[0 .. 4] / 2^20.
//   k > 0 and record[k - 1].status != OK: the estimate has ended.  status = record[k - 1].status, used and seen are
//     this launch's, g = (double)params[0], b = (double)params[1], rss = 0; params are not written.
//   used < min_used: status FEW.
//   det = n * Sxx - Sx * Sx;  not (det / (n * n) > min_var) -- a NaN included: status FLAT (a constant image says nothing
//     about gain).  FEW and FLAT record g, b = the params as they are, rss = 0.
//   g = (n * Sxy - Sx * Sy) / det,  b = (Sy - g * Sx) / n,  rss = (Syy - g * Sxy) - b * Sy (recorded whatever follows);
//   not (gain_min <= g <= gain_max and |b| <= offset_max): status RANGE.
//   otherwise OK: params = ((float)g, (float)b, (float)b * 255.f, 0).
//   Every status but OK leaves params as they were.  record[k] = int64 (status, used, seen), float64 (g, b, rss).
// The launches after a pass that was not OK cannot be skipped (nothing is read back) and still run, as a converged
// alignment's do; they change nothing but their record.  Everything is written with ordinary vector stores.
//
// k_map_exposure_apply, one thread per value of rgb[h,w,3], out of place: t = (params[0] * c) + params[2], out = 0
// where t < 0, 255 where t > 255, t otherwise -- a NaN stays a NaN.
#include "gsloc_internal.h"
#include "map_dev.h"
#include "map_info_dev.h"

namespace gsl {

constexpr int EXPOSURE_THREADS = 256;
constexpr int EXPOSURE_MAX_BLOCKS = 1024;  // k_map_pose_info's grid
constexpr int EXPOSURE_SUMS = 5;           // the fixed-point sums; then the two counts
constexpr int EXPOSURE_SOLVE_THREADS = 64;
static_assert(EXPOSURE_SUMS + 2 == GSL_MAP_EXPOSURE_VALUES, "out is the sums and the two counts");
static_assert(GSL_MAP_EXPOSURE_RECORD_WORDS == 6, "a record is three integers and three doubles");

__device__ static inline bool exposure_in(float t, float lo, float hi) { return t >= lo && t <= hi; }

__global__ __launch_bounds__(EXPOSURE_THREADS) void k_map_exposure_sums(
    const float* __restrict__ means, const float* __restrict__ colors, long long n_rows, const float* __restrict__ w2c,
    float fx, float fy, float cx, float cy, const float* __restrict__ depth, const float* __restrict__ intensity,
    int width, float u_last, float v_last, float keep, float beyond, float near_plane, float sat_lo, float sat_hi,
    float gate, const float* __restrict__ params, unsigned long long* __restrict__ out) {
#pragma clang fp contract(off)
  __shared__ unsigned long long table[GSL_MAP_EXPOSURE_VALUES];
  if ((int)threadIdx.x < GSL_MAP_EXPOSURE_VALUES) table[threadIdx.x] = 0ull;
  __syncthreads();
  const float g0 = params[0], b0 = params[1];
  long long acc[EXPOSURE_SUMS];
#pragma unroll
  for (int i = 0; i < EXPOSURE_SUMS; ++i) acc[i] = 0;
  uint32_t n_used = 0u, n_seen = 0u;  // the wave's: wave-uniform
  const long long stride = (long long)gridDim.x * EXPOSURE_THREADS;
  // the trip count is the workgroup's: every lane of a wave reaches every ballot
  for (long long base = (long long)blockIdx.x * EXPOSURE_THREADS; base < n_rows; base += stride) {
    const long long g = base + threadIdx.x;
    const bool live = g < n_rows;
    float3 row = {0.f, 0.f, 0.f};
    if (live) row = map_load_row(means, g);
    const MapPixel p = map_project(w2c, row, fx, fy, cx, cy);
    bool seen = live && p.z > near_plane && map_inside(p, u_last, v_last);
    bool used = false;
    if (seen) {  // the index is inside
      const size_t at = (size_t)(int)p.vf * (size_t)width + (size_t)(int)p.uf;
      const float d0 = depth[at];
      seen = d0 > 0.f && d0 < INFINITY && d0 * keep <= p.z && p.z <= d0 * beyond;
      if (seen) {
        const float3 c = map_load_row(colors, g);
        const float Yi = (0.299f * c.x + 0.587f * c.y) + 0.114f * c.z;
        const float Y0 = intensity[at];
        if (exposure_in(Yi, sat_lo, sat_hi) && exposure_in(Y0, sat_lo, sat_hi) &&
            fabsf((g0 * Y0 + b0) - Yi) <= gate) {
          used = true;
          acc[0] += info_fix(Y0, Y0);
          acc[1] += info_fix(Y0, 1.f);
          acc[2] += info_fix(Y0, Yi);
          acc[3] += info_fix(Yi, 1.f);
          acc[4] += info_fix(Yi, Yi);
        }
      }
    }
    n_seen += (uint32_t)__popcll(__ballot(seen));
    n_used += (uint32_t)__popcll(__ballot(used));
  }
  // per wave, then LDS
  const bool first_lane = (threadIdx.x & 63) == 0;
#pragma unroll
  for (int i = 0; i < EXPOSURE_SUMS; ++i) {
    long long v = acc[i];
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off);
    if (first_lane && v != 0) atomicAdd(&table[i], (unsigned long long)v);
  }
  if (first_lane && n_seen != 0u) {
    atomicAdd(&table[EXPOSURE_SUMS + 1], (unsigned long long)n_seen);
    if (n_used != 0u) atomicAdd(&table[EXPOSURE_SUMS], (unsigned long long)n_used);
  }
  __syncthreads();
  if ((int)threadIdx.x < GSL_MAP_EXPOSURE_VALUES) {
    const unsigned long long c = table[threadIdx.x];
    if (c != 0ull) atomicAdd(&out[threadIdx.x], c);
  }
}

__global__ __launch_bounds__(EXPOSURE_SOLVE_THREADS) void k_map_exposure_init(float* __restrict__ params) {
  if (threadIdx.x < 4) params[threadIdx.x] = threadIdx.x == 0 ? 1.f : 0.f;
}

__global__ __launch_bounds__(EXPOSURE_SOLVE_THREADS) void k_map_exposure_solve(
    const long long* __restrict__ sums, int k, long long min_used, double gain_min, double gain_max, double offset_max,
    double min_var, float* __restrict__ params, long long* __restrict__ record) {
#pragma clang fp contract(off)
  if (threadIdx.x != 0) return;
  constexpr double ONE = 1048576.0;
  const long long used = sums[5], seen = sums[6];
  const double n = (double)used;
  const double Sxx = (double)sums[0] / ONE, Sx = (double)sums[1] / ONE, Sxy = (double)sums[2] / ONE;
  const double Sy = (double)sums[3] / ONE, Syy = (double)sums[4] / ONE;
  long long* rec = record + (size_t)k * GSL_MAP_EXPOSURE_RECORD_WORDS;
  long long status = GSL_MAP_EXPOSURE_OK;
  double g = (double)params[0], b = (double)params[1], rss = 0.0;
  if (k > 0 && rec[-GSL_MAP_EXPOSURE_RECORD_WORDS] != GSL_MAP_EXPOSURE_OK) {
    status = rec[-GSL_MAP_EXPOSURE_RECORD_WORDS];
  } else if (used < min_used) {
    status = GSL_MAP_EXPOSURE_FEW;
  } else {
    const double det = n * Sxx - Sx * Sx;
    if (!(det / (n * n) > min_var)) {
      status = GSL_MAP_EXPOSURE_FLAT;
    } else {
      g = (n * Sxy - Sx * Sy) / det;
      b = (Sy - g * Sx) / n;
      rss = (Syy - g * Sxy) - b * Sy;
      if (!(g >= gain_min && g <= gain_max && fabs(b) <= offset_max)) {
        status = GSL_MAP_EXPOSURE_RANGE;
      } else {
        const float bf = (float)b;
        params[0] = (float)g;
        params[1] = bf;
        params[2] = bf * 255.f;
        params[3] = 0.f;
      }
    }
  }
  rec[0] = status;
  rec[1] = used;
  rec[2] = seen;
  double* recd = (double*)(rec + 3);
  recd[0] = g;
  recd[1] = b;
  recd[2] = rss;
}

__global__ __launch_bounds__(EXPOSURE_THREADS) void k_map_exposure_apply(const float* __restrict__ rgb, long long n,
                                                                        const float* __restrict__ params,
                                                                        float* __restrict__ out) {
#pragma clang fp contract(off)
  const long long i = (long long)blockIdx.x * EXPOSURE_THREADS + threadIdx.x;
  if (i >= n) return;
  const float t = (params[0] * rgb[i]) + params[2];
  out[i] = t < 0.f ? 0.f : t > 255.f ? 255.f : t;
}

}  // namespace gsl

extern "C" int gsl_map_exposure_values(void) { return GSL_MAP_EXPOSURE_VALUES; }

extern "C" int gsl_map_exposure_estimate(const float* means, const float* colors, int64_t n_rows, const float* w2c,
                                         float fx, float fy, float cx, float cy, const float* depth,
                                         const float* intensity, int width, int height, float keep, float beyond,
                                         float near_plane, float sat_lo, float sat_hi, float max_residual, int passes,
                                         int min_used, double gain_min, double gain_max, double offset_max,
                                         double min_var, int64_t* sums, float* params, void* record, void* stream) {
  if (!means || !colors || !w2c || !depth || !intensity || !sums || !params || !record) return GSL_ERR_BAD_ARG;
  if (!gsl::map_rows_ok(n_rows)) return GSL_ERR_BAD_ARG;
  if (!gsl::map_image_ok(width, height) || !gsl::map_focal_ok(fx, fy)) return GSL_ERR_BAD_ARG;
  if (!(keep > 0.f && keep <= 1.f) || !(beyond >= 1.f && beyond < INFINITY)) return GSL_ERR_BAD_ARG;
  if (!(sat_lo >= 0.f && sat_lo < sat_hi && sat_hi <= 1.f)) return GSL_ERR_BAD_ARG;  // what bounds the sums
  if (!(max_residual >= 0.f && max_residual < INFINITY)) return GSL_ERR_BAD_ARG;
  if (passes < 1 || passes > GSL_MAP_EXPOSURE_MAX_PASSES || min_used < 1) return GSL_ERR_BAD_ARG;
  if (!(gain_min > 0.0 && gain_min <= 1.0 && gain_max >= 1.0 && gain_max < (double)INFINITY)) return GSL_ERR_BAD_ARG;
  if (!(offset_max >= 0.0 && offset_max < (double)INFINITY) || !(min_var >= 0.0 && min_var < (double)INFINITY))
    return GSL_ERR_BAD_ARG;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(gsl::k_map_exposure_init, dim3(1), dim3(gsl::EXPOSURE_SOLVE_THREADS), 0, st, params);
  GSL_CHECK_LAUNCH();
  const long long blocks = (n_rows + gsl::EXPOSURE_THREADS - 1) / gsl::EXPOSURE_THREADS;
  const int nb = (int)(blocks < gsl::EXPOSURE_MAX_BLOCKS ? blocks : gsl::EXPOSURE_MAX_BLOCKS);
  for (int k = 0; k < passes; ++k) {
    const int rc = gsl::zero_u32(sums, (size_t)2 * GSL_MAP_EXPOSURE_VALUES, st);
    if (rc != GSL_OK) return rc;
    hipLaunchKernelGGL(gsl::k_map_exposure_sums, dim3(nb), dim3(gsl::EXPOSURE_THREADS), 0, st, means, colors,
                       (long long)n_rows, w2c, fx, fy, cx, cy, depth, intensity, width, (float)(width - 1),
                       (float)(height - 1), keep, beyond, near_plane, sat_lo, sat_hi, k == 0 ? INFINITY : max_residual,
                       (const float*)params, (unsigned long long*)sums);
    GSL_CHECK_LAUNCH();
    hipLaunchKernelGGL(gsl::k_map_exposure_solve, dim3(1), dim3(gsl::EXPOSURE_SOLVE_THREADS), 0, st,
                       (const long long*)sums, k, (long long)min_used, gain_min, gain_max, offset_max, min_var, params,
                       (long long*)record);
    GSL_CHECK_LAUNCH();
  }
  return GSL_OK;
}

extern "C" int gsl_map_exposure_apply(const float* rgb, int width, int height, const float* params, float* out,
                                      void* stream) {
  if (!rgb || !params || !out || !gsl::map_image_ok(width, height)) return GSL_ERR_BAD_ARG;
  const long long n = (long long)width * height * 3;
  hipLaunchKernelGGL(gsl::k_map_exposure_apply,
                     dim3((unsigned)((n + gsl::EXPOSURE_THREADS - 1) / gsl::EXPOSURE_THREADS)),
                     dim3(gsl::EXPOSURE_THREADS), 0, (hipStream_t)stream, rgb, n, params, out);
  GSL_CHECK_LAUNCH();
  return GSL_OK;
}
