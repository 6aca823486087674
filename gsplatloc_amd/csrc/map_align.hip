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
// The code of that sequence is align_step of map_align_dev.h, the one copy: map_align_batch.hip runs it for several poses.
// gsl_map_pose_align_photo is the same sequence with the sums of map_photo.hip (geometry plus colour) in place of
// k_map_pose_info's: the 30 integers have one layout, and nothing here reads more than them.
#include "gsloc_internal.h"
#include "map_align_dev.h"
#include "map_dev.h"
#include "map_info_dev.h"

namespace gsl {

__global__ __launch_bounds__(ALIGN_THREADS) void k_map_align_init(const float* __restrict__ w2c, float* __restrict__ work,
                                                                  double* __restrict__ state) {
  align_init(w2c, work, state, (int)threadIdx.x);
}

__global__ __launch_bounds__(ALIGN_THREADS) void k_map_align_step(
    const long long* __restrict__ sums_in, int k, double damping, long long min_used, double max_rot, double max_trans,
    double eps_rot, double eps_trans, float* __restrict__ work, double* __restrict__ state,
    long long* __restrict__ history) {
#pragma clang fp contract(off)
  if (threadIdx.x != 0) return;
  align_step(sums_in, k, damping, min_used, max_rot, max_trans, eps_rot, eps_trans, work, state, history);
}

}  // namespace gsl

extern "C" int gsl_map_align_max_steps(void) { return GSL_MAP_ALIGN_MAX_STEPS; }

// The launch sequence of gsl_map_pose_align for checked arguments; photo NULL: the geometric sums, otherwise the
// photometric ones (map_photo.hip) in their place -- the init and step kernels do not know which.
static int map_pose_align_run(const float* means, int64_t n_rows, const float* w2c, float fx, float fy, float cx,
                              float cy, const float* depth, int width, int height, float keep, float beyond, float kappa,
                              float near_plane, int max_steps, double damping, int min_used, double max_rot,
                              double max_trans, double eps_rot, double eps_trans, int64_t* sums, float* work, void* state,
                              void* history, const gsl::InfoPhoto* photo, hipStream_t st) {
  hipLaunchKernelGGL(gsl::k_map_align_init, dim3(1), dim3(gsl::ALIGN_THREADS), 0, st, w2c, work, (double*)state);
  GSL_CHECK_LAUNCH();
  for (int k = 0; k < max_steps; ++k) {
    const int rc = photo ? gsl::map_pose_info_photo_launch(means, n_rows, work, fx, fy, cx, cy, depth, width, height,
                                                           keep, beyond, kappa, near_plane, sums, *photo, nullptr, st)
                         : gsl::map_pose_info_launch(means, n_rows, work, fx, fy, cx, cy, depth, width, height, keep,
                                                     beyond, kappa, near_plane, sums, st);
    if (rc != GSL_OK) return rc;
    hipLaunchKernelGGL(gsl::k_map_align_step, dim3(1), dim3(gsl::ALIGN_THREADS), 0, st, (const long long*)sums, k,
                       damping, (long long)min_used, max_rot, max_trans, eps_rot, eps_trans, work, (double*)state,
                       (long long*)history);
    GSL_CHECK_LAUNCH();
  }
  return GSL_OK;
}

extern "C" int gsl_map_pose_align(const float* means, int64_t n_rows, const float* w2c, float fx, float fy, float cx,
                                  float cy, const float* depth, int width, int height, float keep, float beyond,
                                  float kappa, float near_plane, int max_steps, double damping, int min_used,
                                  double max_rot, double max_trans, double eps_rot, double eps_trans, int64_t* sums,
                                  float* work, void* state, void* history, void* stream) {
  if (!w2c || !sums || !work || !state || !history) return GSL_ERR_BAD_ARG;
  if (!gsl::align_args_ok(means, n_rows, fx, fy, cx, cy, depth, width, height, keep, beyond, kappa, max_steps, damping,
                          min_used, max_rot, max_trans, eps_rot, eps_trans))
    return GSL_ERR_BAD_ARG;
  return map_pose_align_run(means, n_rows, w2c, fx, fy, cx, cy, depth, width, height, keep, beyond, kappa, near_plane,
                            max_steps, damping, min_used, max_rot, max_trans, eps_rot, eps_trans, sums, work, state,
                            history, nullptr, (hipStream_t)stream);
}

extern "C" int gsl_map_pose_align_photo(const float* means, int64_t n_rows, const float* w2c, float fx, float fy,
                                        float cx, float cy, const float* depth, int width, int height, float keep,
                                        float beyond, float kappa, float near_plane, int max_steps, double damping,
                                        int min_used, double max_rot, double max_trans, double eps_rot, double eps_trans,
                                        int64_t* sums, float* work, void* state, void* history, const float* colors,
                                        const float* intensity, float photo_scale, float photo_max_residual,
                                        void* stream) {
  if (!w2c || !sums || !work || !state || !history) return GSL_ERR_BAD_ARG;
  if (!gsl::align_args_ok(means, n_rows, fx, fy, cx, cy, depth, width, height, keep, beyond, kappa, max_steps, damping,
                          min_used, max_rot, max_trans, eps_rot, eps_trans))
    return GSL_ERR_BAD_ARG;
  const gsl::InfoPhoto photo = {colors, intensity, photo_scale, photo_max_residual};
  if (!gsl::info_photo_args_ok(photo)) return GSL_ERR_BAD_ARG;
  if (n_rows > gsl_map_info_photo_max_rows(fx, fy, cx, cy, width, height, keep, photo_scale, photo_max_residual))
    return GSL_ERR_BAD_ARG;  // a sum could overflow
  return map_pose_align_run(means, n_rows, w2c, fx, fy, cx, cy, depth, width, height, keep, beyond, kappa, near_plane,
                            max_steps, damping, min_used, max_rot, max_trans, eps_rot, eps_trans, sums, work, state,
                            history, &photo, (hipStream_t)stream);
}
