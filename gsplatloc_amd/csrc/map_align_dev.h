// Frame-to-map localisation, the Gauss-Newton step of a pose alignment, the one copy: what one thread does with the 30
// sums of a pose, in the order written at the top of map_align.hip (float64, no contraction, one rounding per operation;
// tests/map_align_ref.py is the same sequence in numpy).  k_map_align_init / k_map_align_step (map_align.hip) are these
// functions for one pose; the batched alignment (map_align_batch.hip) runs them for one pose per thread.
#pragma once
#include "gsloc_common.h"
#include "map_dev.h"

namespace gsl {

constexpr int ALIGN_THREADS = 64;
constexpr int ALIGN_POSE = 12;  // words of state that hold P; then steps_taken, done
static_assert(ALIGN_POSE + 2 == GSL_MAP_ALIGN_STATE_WORDS, "state is the pose and two integers");
static_assert(GSL_MAP_ALIGN_ROW_WORDS == 10, "a history row is four integers and xi");
static_assert(sizeof(double) == 8 && sizeof(long long) == 8, "8-byte words");

// What gsl_map_pose_align and gsl_map_pose_align_batch refuse alike before any launch, their buffers apart: whatever
// gsl_map_pose_info refuses of the rows, the image and the row rule, and the iteration's own parameters.
static inline bool align_args_ok(const float* means, int64_t n_rows, float fx, float fy, float cx, float cy,
                                 const float* depth, int width, int height, float keep, float beyond, float kappa,
                                 int max_steps, double damping, int min_used, double max_rot, double max_trans,
                                 double eps_rot, double eps_trans) {
  if (!means || !depth || !map_rows_ok(n_rows)) return false;
  if (!map_image_ok(width, height) || !map_focal_ok(fx, fy)) return false;
  if (!(keep > 0.f && keep <= 1.f) || !(beyond >= 1.f && beyond < INFINITY)) return false;
  if (!(kappa >= 0.f && kappa < INFINITY)) return false;
  if (n_rows > gsl_map_info_max_rows(fx, fy, cx, cy, width, height, keep)) return false;  // a sum could overflow
  if (max_steps < 1 || max_steps > GSL_MAP_ALIGN_MAX_STEPS || min_used < 7) return false;
  if (!(damping >= 0.0 && damping < (double)INFINITY)) return false;
  if (!(max_rot > 0.0 && max_rot < (double)INFINITY) || !(max_trans > 0.0 && max_trans < (double)INFINITY)) return false;
  return eps_rot >= 0.0 && eps_rot < (double)INFINITY && eps_trans >= 0.0 && eps_trans < (double)INFINITY;
}

// Thread t of 18 or more: P = the exact widening of w2c's 12 entries, work = them and (0, 0, 0, 1), steps_taken = done = 0.
__device__ static inline void align_init(const float* __restrict__ w2c, float* __restrict__ work,
                                         double* __restrict__ state, int t) {
  if (t < 16) {
    const float v = t < 12 ? w2c[t] : (t == 15 ? 1.f : 0.f);
    work[t] = v;
    if (t < ALIGN_POSE) state[t] = (double)v;
  }
  if (t == 16 || t == 17) ((long long*)state)[ALIGN_POSE + (t - 16)] = 0ll;
}

__device__ static inline void align_row(long long* __restrict__ row, long long status, const long long* sums,
                                        const double* xi) {
  row[0] = status;
  row[1] = sums[28];
  row[2] = sums[29];
  row[3] = sums[27];
  double* x = (double*)(row + 4);
#pragma unroll
  for (int i = 0; i < 6; ++i) x[i] = xi ? xi[i] : 0.0;
}

// Iteration k of one pose, by one thread.  Writes history row k, and what the status says of work, state and its two
// integers: done goes from 0 to 1 with every status but STEPPED.  Returns the status of the row.
__device__ static inline long long align_step(const long long* __restrict__ sums_in, int k, double damping,
                                              long long min_used, double max_rot, double max_trans, double eps_rot,
                                              double eps_trans, float* __restrict__ work, double* __restrict__ state,
                                              long long* __restrict__ history) {
#pragma clang fp contract(off)
  long long sums[GSL_MAP_INFO_VALUES];
#pragma unroll
  for (int i = 0; i < GSL_MAP_INFO_VALUES; ++i) sums[i] = sums_in[i];
  long long* flags = (long long*)state + ALIGN_POSE;  // steps_taken, done
  long long* row = history + (size_t)k * GSL_MAP_ALIGN_ROW_WORDS;
  if (flags[1] != 0) {  // k > 0: done is 0 after align_init
    const long long before = (row - GSL_MAP_ALIGN_ROW_WORDS)[0];
    align_row(row, before, sums, nullptr);
    return before;
  }
  const long long used = sums[28];
  if (used < min_used) {
    align_row(row, GSL_MAP_ALIGN_FEW, sums, nullptr);
    flags[1] = 1;
    return GSL_MAP_ALIGN_FEW;
  }
  double A[6][6], b[6];
  {
    int slot = 0;
#pragma unroll
    for (int a = 0; a < 6; ++a)
#pragma unroll
      for (int c = a; c < 6; ++c) {
        const double v = (double)sums[slot++] / 1048576.0;
        A[a][c] = v;
        A[c][a] = v;
      }
  }
  const double lambda = damping * (double)used;
#pragma unroll
  for (int a = 0; a < 6; ++a) {
    A[a][a] = A[a][a] + lambda;
    b[a] = -((double)sums[21 + a] / 1048576.0);
  }
  double L[6][6], D[6];
  bool singular = false;
#pragma unroll
  for (int j = 0; j < 6; ++j) {
    double d = A[j][j];
#pragma unroll
    for (int q = 0; q < j; ++q) d = d - (L[j][q] * L[j][q]) * D[q];
    if (!(d > 0.0)) singular = true;
    D[j] = d;
#pragma unroll
    for (int i = j + 1; i < 6; ++i) {
      double s = A[i][j];
#pragma unroll
      for (int q = 0; q < j; ++q) s = s - (L[i][q] * L[j][q]) * D[q];
      L[i][j] = s / d;
    }
  }
  if (singular) {  // some pivot was not above 0; what followed it is garbage and is not used
    align_row(row, GSL_MAP_ALIGN_SINGULAR, sums, nullptr);
    flags[1] = 1;
    return GSL_MAP_ALIGN_SINGULAR;
  }
  double z[6], x[6];
#pragma unroll
  for (int i = 0; i < 6; ++i) {
    double v = b[i];
#pragma unroll
    for (int q = 0; q < i; ++q) v = v - L[i][q] * z[q];
    z[i] = v;
  }
#pragma unroll
  for (int i = 5; i >= 0; --i) {
    double v = z[i] / D[i];
#pragma unroll
    for (int q = i + 1; q < 6; ++q) v = v - L[q][i] * x[q];
    x[i] = v;
  }
  const double ww = (x[0] * x[0] + x[1] * x[1]) + x[2] * x[2];
  const double vv = (x[3] * x[3] + x[4] * x[4]) + x[5] * x[5];
  if (!(ww <= max_rot * max_rot && vv <= max_trans * max_trans)) {
    align_row(row, GSL_MAP_ALIGN_TOO_FAR, sums, x);
    flags[1] = 1;
    return GSL_MAP_ALIGN_TOO_FAR;
  }
  const double a0 = x[0] * 0.5, a1 = x[1] * 0.5, a2 = x[2] * 0.5;
  const double s = (a0 * a0 + a1 * a1) + a2 * a2;
  const double c = 1.0 - s, den = 1.0 + s;
  const double t00 = (a0 * a0) * 2.0, t11 = (a1 * a1) * 2.0, t22 = (a2 * a2) * 2.0;
  const double t01 = (a0 * a1) * 2.0, t02 = (a0 * a2) * 2.0, t12 = (a1 * a2) * 2.0;
  const double u0 = a0 * 2.0, u1 = a1 * 2.0, u2 = a2 * 2.0;
  const double R[3][3] = {{(c + t00) / den, (t01 - u2) / den, (t02 + u1) / den},
                          {(t01 + u2) / den, (c + t11) / den, (t12 - u0) / den},
                          {(t02 - u1) / den, (t12 + u0) / den, (c + t22) / den}};
  double P[3][4], Q[3][4];
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) P[i][j] = state[i * 4 + j];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
#pragma unroll
    for (int j = 0; j < 4; ++j) Q[i][j] = (R[i][0] * P[0][j] + R[i][1] * P[1][j]) + R[i][2] * P[2][j];
    Q[i][3] = Q[i][3] + x[3 + i];
  }
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      state[i * 4 + j] = Q[i][j];
      work[i * 4 + j] = (float)Q[i][j];  // round to nearest even
    }
  flags[0] = flags[0] + 1;
  const bool converged = ww <= eps_rot * eps_rot && vv <= eps_trans * eps_trans;
  const long long status = converged ? GSL_MAP_ALIGN_CONVERGED : GSL_MAP_ALIGN_STEPPED;
  align_row(row, status, sums, x);
  if (converged) flags[1] = 1;
  return status;
}

}  // namespace gsl
