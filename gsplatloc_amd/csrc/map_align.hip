// Frame-to-map localisation: a pose aligned to the map by Gauss-Newton on the device (gsplatloc_amd/mapping.py:
// align_pose).  k_map_pose_info (map_info.hip) sums the point-to-plane normal equations of a pose over the map's rows in
// one launch; here a one-thread kernel takes the damped Gauss-Newton step from those 30 integers, moves the pose and
// writes the float32 copy that the next launch of k_map_pose_info reads.  gsl_map_pose_align is one fixed sequence of
// launches on the given stream -- k_map_align_init, then max_steps times (zero_u32 of the sums, k_map_pose_info,
// k_map_align_step) -- with no allocation, no synchronisation and no read-back: the host reads the state and the history
// when it wants them.  k_map_pose_info cannot read ``done``: a pose that has converged still pays the remaining launches
// (NOTES.md, "Pose alignment"), and k_map_align_step only copies the status.
//
// The buffers, all on the device: sums[30] int64 (map_info.hip's out); work[16] float32, the working world-to-camera
// matrix, row-major, row 3 = (0, 0, 0, 1); state[GSL_MAP_ALIGN_STATE_WORDS] 8-byte words: the pose P, the upper 3 x 4 of
// the world-to-camera matrix row-major as 12 float64, then int64 steps_taken (the steps applied) and int64 done;
// history[max_steps][GSL_MAP_ALIGN_ROW_WORDS] 8-byte words: row k = int64 (status, used, tested, rss_fixed = sums[27])
// of iteration k, then float64 xi[6] = (omega [rad], upsilon [m]).  k_map_align_init: P = the exact widening of the 12
// float32 entries of the given w2c, work = its 12 entries and (0, 0, 0, 1), steps_taken = done = 0.
//
// k_map_align_step, iteration k: float64, no contraction, every operation rounded once in the order written here
// (tests/map_align_ref.py is the same sequence in numpy and gives the same bits):
//   the 30 integers are read.  If done: status = history[k - 1].status, used, tested, rss_fixed from the sums, xi = 0;
//     nothing else is written.
//   used < min_used: status FEW, xi = 0, done = 1.
//   A_ab = (double)sums[slot(a, b)] / 2^20 for a <= b (map_info.hip's upper triangle), mirrored below the diagonal;
//     lambda = damping * (double)used;  A_aa = A_aa + lambda;  b_a = -((double)sums[21 + a] / 2^20).
//   LDL^T, for j = 0 .. 5:  d = A_jj;  for k = 0 .. j - 1 in order: d = d - (L_jk * L_jk) * D_k;
//     a pivot that is not d > 0 (a NaN included): status SINGULAR, xi = 0, done = 1;  D_j = d;
//     for i = j + 1 .. 5:  s = A_ij;  for k = 0 .. j - 1 in order: s = s - (L_ik * L_jk) * D_k;  L_ij = s / d.
//   Solve: for i = 0 .. 5:  z_i = b_i;  for k = 0 .. i - 1 in order: z_i = z_i - L_ik * z_k;   y_i = z_i / D_i;
//     for i = 5 .. 0:  x_i = y_i;  for k = i + 1 .. 5 in order: x_i = x_i - L_ki * x_k;   xi = x,
//     omega = (x_0, x_1, x_2), upsilon = (x_3, x_4, x_5).
//   ww = (omega_0 omega_0 + omega_1 omega_1) + omega_2 omega_2, vv likewise of upsilon.  Not (ww <= max_rot * max_rot and
//     vv <= max_trans * max_trans) -- a NaN included: status TOO_FAR, xi as solved, done = 1, the pose is not touched.
//   Retraction, the Cayley map and NOT the exponential: a = omega * 0.5, s = (a_0 a_0 + a_1 a_1) + a_2 a_2, c = 1 - s,
//     den = 1 + s, t_ij = (a_i * a_j) * 2, u_i = a_i * 2:
//       R = [ (c + t_00) / den,   (t_01 - u_2) / den,  (t_02 + u_1) / den ]
//           [ (t_01 + u_2) / den, (c + t_11) / den,    (t_12 - u_0) / den ]
//           [ (t_02 - u_1) / den, (t_12 + u_0) / den,  (c + t_22) / den   ]
//     = ((1 - s) I + 2 a a^T + 2 [a]x) / (1 + s): an exact rotation about omega for every omega (by 2 atan(|omega| / 2),
//     which is |omega| up to |omega|^3 / 12), so it agrees with exp to first order, and it is the identity exactly when
//     omega = 0: the iteration has the fixed point of the exponential's.  It needs + - x / only -- no sine and no
//     cosine, whose device and numpy versions differ in the last bit -- which is what lets the mirror give the same
//     bits.  (The host's apply_twist stays the exponential.)
//     P'_ij = (R_i0 P_0j + R_i1 P_1j) + R_i2 P_2j for j = 0 .. 2, P'_i3 = ((R_i0 P_03 + R_i1 P_13) + R_i2 P_23) + upsilon_i:
//     P <- [R | upsilon] P, the left perturbation of map_info.hip.
//   work = (float)P', round to nearest even; steps_taken = steps_taken + 1.
//   ww <= eps_rot * eps_rot and vv <= eps_trans * eps_trans: status CONVERGED, done = 1 (the step has been applied);
//     otherwise status STEPPED.
// One workgroup of one wave; lane 0 does the work and the other lanes leave at once.  Every loop is unrolled, L, D and
// the rest live in registers (no scratch).  Everything is written with ordinary vector stores.
#include "gsloc_internal.h"
#include "map_dev.h"

namespace gsl {

constexpr int ALIGN_THREADS = 64;
constexpr int ALIGN_POSE = 12;  // words of state that hold P; then steps_taken, done
static_assert(ALIGN_POSE + 2 == GSL_MAP_ALIGN_STATE_WORDS, "state is the pose and two integers");
static_assert(GSL_MAP_ALIGN_ROW_WORDS == 10, "a history row is four integers and xi");
static_assert(sizeof(double) == 8 && sizeof(long long) == 8, "8-byte words");

__global__ __launch_bounds__(ALIGN_THREADS) void k_map_align_init(const float* __restrict__ w2c, float* __restrict__ work,
                                                                  double* __restrict__ state) {
  const int t = (int)threadIdx.x;
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

__global__ __launch_bounds__(ALIGN_THREADS) void k_map_align_step(
    const long long* __restrict__ sums_in, int k, double damping, long long min_used, double max_rot, double max_trans,
    double eps_rot, double eps_trans, float* __restrict__ work, double* __restrict__ state,
    long long* __restrict__ history) {
#pragma clang fp contract(off)
  if (threadIdx.x != 0) return;
  long long sums[GSL_MAP_INFO_VALUES];
#pragma unroll
  for (int i = 0; i < GSL_MAP_INFO_VALUES; ++i) sums[i] = sums_in[i];
  long long* flags = (long long*)state + ALIGN_POSE;  // steps_taken, done
  long long* row = history + (size_t)k * GSL_MAP_ALIGN_ROW_WORDS;
  if (flags[1] != 0) {  // k > 0: done is 0 after k_map_align_init
    align_row(row, (row - GSL_MAP_ALIGN_ROW_WORDS)[0], sums, nullptr);
    return;
  }
  const long long used = sums[28];
  if (used < min_used) {
    align_row(row, GSL_MAP_ALIGN_FEW, sums, nullptr);
    flags[1] = 1;
    return;
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
    return;
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
    return;
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
  align_row(row, converged ? GSL_MAP_ALIGN_CONVERGED : GSL_MAP_ALIGN_STEPPED, sums, x);
  if (converged) flags[1] = 1;
}

}  // namespace gsl

extern "C" int gsl_map_align_max_steps(void) { return GSL_MAP_ALIGN_MAX_STEPS; }

extern "C" int gsl_map_pose_align(const float* means, int64_t n_rows, const float* w2c, float fx, float fy, float cx,
                                  float cy, const float* depth, int width, int height, float keep, float beyond,
                                  float kappa, float near_plane, int max_steps, double damping, int min_used,
                                  double max_rot, double max_trans, double eps_rot, double eps_trans, int64_t* sums,
                                  float* work, void* state, void* history, void* stream) {
  if (!means || !w2c || !depth || !sums || !work || !state || !history) return GSL_ERR_BAD_ARG;
  if (!gsl::map_rows_ok(n_rows)) return GSL_ERR_BAD_ARG;
  if (!gsl::map_image_ok(width, height) || !gsl::map_focal_ok(fx, fy)) return GSL_ERR_BAD_ARG;
  if (!(keep > 0.f && keep <= 1.f) || !(beyond >= 1.f && beyond < INFINITY)) return GSL_ERR_BAD_ARG;
  if (!(kappa >= 0.f && kappa < INFINITY)) return GSL_ERR_BAD_ARG;
  if (n_rows > gsl_map_info_max_rows(fx, fy, cx, cy, width, height, keep)) return GSL_ERR_BAD_ARG;  // a sum could overflow
  if (max_steps < 1 || max_steps > GSL_MAP_ALIGN_MAX_STEPS || min_used < 7) return GSL_ERR_BAD_ARG;
  if (!(damping >= 0.0 && damping < (double)INFINITY)) return GSL_ERR_BAD_ARG;
  if (!(max_rot > 0.0 && max_rot < (double)INFINITY) || !(max_trans > 0.0 && max_trans < (double)INFINITY))
    return GSL_ERR_BAD_ARG;
  if (!(eps_rot >= 0.0 && eps_rot < (double)INFINITY) || !(eps_trans >= 0.0 && eps_trans < (double)INFINITY))
    return GSL_ERR_BAD_ARG;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(gsl::k_map_align_init, dim3(1), dim3(gsl::ALIGN_THREADS), 0, st, w2c, work, (double*)state);
  GSL_CHECK_LAUNCH();
  for (int k = 0; k < max_steps; ++k) {
    const int rc = gsl::map_pose_info_launch(means, n_rows, work, fx, fy, cx, cy, depth, width, height, keep, beyond,
                                             kappa, near_plane, sums, st);
    if (rc != GSL_OK) return rc;
    hipLaunchKernelGGL(gsl::k_map_align_step, dim3(1), dim3(gsl::ALIGN_THREADS), 0, st, (const long long*)sums, k,
                       damping, (long long)min_used, max_rot, max_trans, eps_rot, eps_trans, work, (double*)state,
                       (long long*)history);
    GSL_CHECK_LAUNCH();
  }
  return GSL_OK;
}
