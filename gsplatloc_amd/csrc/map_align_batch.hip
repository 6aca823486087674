// Frame-to-map localisation: several poses aligned to the map in one call (gsplatloc_amd/mapping.py: align_poses), each
// by the Gauss-Newton iteration of map_align.hip, and a pose that has finished stops paying for its sums.
// gsl_map_pose_align_batch is one fixed sequence of launches on the given stream -- k_map_batch_init, then max_steps
// times (k_map_batch_zero, k_map_batch_info, k_map_batch_step) -- with no allocation, no synchronisation, no read-back
// and no memset node: safe to capture.  The poses share the rows, the depth frame and every parameter.
//
// The buffers are map_align.hip's per pose, pose-major: sums[n_poses][30] int64, work[n_poses][16] float32,
// state[n_poses][GSL_MAP_ALIGN_STATE_WORDS], history[n_poses][max_steps][GSL_MAP_ALIGN_ROW_WORDS].
//
// done, the last word of a pose's state, has three values here: 0 running; 1 finished, the sums at its final pose still
// to be taken; 2 closed.  Iteration k:
//   k_map_batch_zero  zeroes the 30 sums of every pose that is not closed (one thread per sum).
//   k_map_batch_info  blockIdx.y is the pose; a workgroup reads done and leaves when the pose is closed, otherwise it is
//                     a workgroup of k_map_pose_info at work[pose] (info_sum_rows of map_info_dev.h, the one copy; int64
//                     fixed-point atomics, so no sum depends on an order).
//   k_map_batch_step  one thread per pose.  Closed: row k = the four integers of row k - 1 and xi = 0, nothing is read
//                     but that row.  Otherwise align_step of map_align_dev.h (the one copy of map_align.hip's sequence,
//                     float64, no contraction) and then: done was 1 -- the row just written is the closing one, the
//                     status of row k - 1 with the sums at the final pose -- done = 2;  done was 0 and the status is FEW,
//                     SINGULAR or TOO_FAR -- the pose did not move, the sums are at the final pose -- done = 2;
//                     CONVERGED leaves the 1 that align_step set: the next iteration closes the pose.
// gsl_map_pose_align recomputes identical integers at an unchanged pose, so state (done apart), work and every history
// row are bit for bit what it leaves for that pose alone; after the call sums[p] are the normal equations at work[p],
// unless the pose converged on the last iteration and done is left at 1.  Ordinary vector stores only.
// gsl_map_pose_align_batch_photo is the same sequence with k_map_batch_photo_info -- the sums of map_photo.hip, geometry
// plus colour -- in place of k_map_batch_info.
#include "gsloc_internal.h"
#include "map_align_dev.h"
#include "map_info_dev.h"

namespace gsl {

constexpr int BATCH_MAX_POSES = GSL_MAP_ALIGN_BATCH_MAX_POSES;
static_assert(BATCH_MAX_POSES <= ALIGN_THREADS, "one thread per pose takes the step");
static_assert(BATCH_MAX_POSES * GSL_MAP_INFO_VALUES <= 512, "one workgroup zeroes the sums");
constexpr int BATCH_ZERO_THREADS = 512;
// the sums' grid: per pose that of k_map_pose_info, so that one pose costs what the single call's launch does
constexpr int BATCH_INFO_THREADS = 256;
constexpr int BATCH_INFO_MAX_BLOCKS = 1024;

__device__ static inline long long batch_done(const void* state, int pose) {
  return ((const long long*)state)[(size_t)pose * GSL_MAP_ALIGN_STATE_WORDS + ALIGN_POSE + 1];
}

__global__ __launch_bounds__(ALIGN_THREADS) void k_map_batch_init(const float* __restrict__ w2c, float* __restrict__ work,
                                                                  double* __restrict__ state) {
  const size_t p = blockIdx.x;
  align_init(w2c + 16 * p, work + 16 * p, state + GSL_MAP_ALIGN_STATE_WORDS * p, (int)threadIdx.x);
}

__global__ __launch_bounds__(BATCH_ZERO_THREADS) void k_map_batch_zero(const double* __restrict__ state, int n_poses,
                                                                        long long* __restrict__ sums) {
  const int t = (int)threadIdx.x, p = t / GSL_MAP_INFO_VALUES;
  if (p < n_poses && batch_done(state, p) != 2) sums[t] = 0ll;
}

__global__ __launch_bounds__(BATCH_INFO_THREADS) void k_map_batch_info(
    const float* __restrict__ means, long long n_rows, const float* __restrict__ work, const double* __restrict__ state,
    float fx, float fy, float cx, float cy, const float* __restrict__ depth, int width, float u_inner, float v_inner,
    float keep, float beyond, float kappa, float near_plane, unsigned long long* __restrict__ sums) {
#pragma clang fp contract(off)
  const int p = (int)blockIdx.y;
  if (batch_done(state, p) == 2) return;  // the workgroup's: every thread leaves
  info_sum_rows<BATCH_INFO_THREADS, false>(means, n_rows, work + 16 * (size_t)p, fx, fy, cx, cy, depth, width, u_inner,
                                           v_inner, keep, beyond, kappa, near_plane,
                                           sums + GSL_MAP_INFO_VALUES * (size_t)p, nullptr, nullptr, 0.f, 0.f, nullptr);
}

// k_map_batch_info with the photometric term of map_photo.hip in the sums (info_sum_rows with PHOTO; no extra).
__global__ __launch_bounds__(BATCH_INFO_THREADS) void k_map_batch_photo_info(
    const float* __restrict__ means, long long n_rows, const float* __restrict__ work, const double* __restrict__ state,
    float fx, float fy, float cx, float cy, const float* __restrict__ depth, int width, float u_inner, float v_inner,
    float keep, float beyond, float kappa, float near_plane, unsigned long long* __restrict__ sums,
    const float* __restrict__ colors, const float* __restrict__ intensity, float photo_scale, float photo_max_residual) {
#pragma clang fp contract(off)
  const int p = (int)blockIdx.y;
  if (batch_done(state, p) == 2) return;  // the workgroup's: every thread leaves
  info_sum_rows<BATCH_INFO_THREADS, true>(means, n_rows, work + 16 * (size_t)p, fx, fy, cx, cy, depth, width, u_inner,
                                          v_inner, keep, beyond, kappa, near_plane,
                                          sums + GSL_MAP_INFO_VALUES * (size_t)p, colors, intensity, photo_scale,
                                          photo_max_residual, nullptr);
}

__global__ __launch_bounds__(ALIGN_THREADS) void k_map_batch_step(
    const long long* __restrict__ sums, int n_poses, int k, int max_steps, double damping, long long min_used,
    double max_rot, double max_trans, double eps_rot, double eps_trans, float* __restrict__ work,
    double* __restrict__ state, long long* __restrict__ history) {
#pragma clang fp contract(off)
  const int p = (int)threadIdx.x;
  if (p >= n_poses) return;
  double* st = state + GSL_MAP_ALIGN_STATE_WORDS * (size_t)p;
  long long* hist = history + (size_t)p * max_steps * GSL_MAP_ALIGN_ROW_WORDS;
  long long* done = (long long*)st + ALIGN_POSE + 1;
  const long long was = *done;
  if (was == 2) {  // k > 0
    long long* row = hist + (size_t)k * GSL_MAP_ALIGN_ROW_WORDS;
#pragma unroll
    for (int i = 0; i < 4; ++i) row[i] = (row - GSL_MAP_ALIGN_ROW_WORDS)[i];
#pragma unroll
    for (int i = 4; i < GSL_MAP_ALIGN_ROW_WORDS; ++i) ((double*)row)[i] = 0.0;
    return;
  }
  const long long status = align_step(sums + GSL_MAP_INFO_VALUES * (size_t)p, k, damping, min_used, max_rot, max_trans,
                                      eps_rot, eps_trans, work + 16 * (size_t)p, st, hist);
  if (was == 1 || (status != GSL_MAP_ALIGN_STEPPED && status != GSL_MAP_ALIGN_CONVERGED)) *done = 2;
}

}  // namespace gsl

extern "C" int gsl_map_align_batch_max_poses(void) { return GSL_MAP_ALIGN_BATCH_MAX_POSES; }

// The launch sequence of gsl_map_pose_align_batch for checked arguments; photo NULL: k_map_batch_info, otherwise
// k_map_batch_photo_info in its place.
static int map_pose_align_batch_run(const float* means, int64_t n_rows, const float* w2c, int n_poses, float fx, float fy,
                                    float cx, float cy, const float* depth, int width, int height, float keep,
                                    float beyond, float kappa, float near_plane, int max_steps, double damping,
                                    int min_used, double max_rot, double max_trans, double eps_rot, double eps_trans,
                                    int64_t* sums, float* work, void* state, void* history,
                                    const gsl::InfoPhoto* photo, hipStream_t st) {
  hipLaunchKernelGGL(gsl::k_map_batch_init, dim3(n_poses), dim3(gsl::ALIGN_THREADS), 0, st, w2c, work, (double*)state);
  GSL_CHECK_LAUNCH();
  const long long blocks = (n_rows + gsl::BATCH_INFO_THREADS - 1) / gsl::BATCH_INFO_THREADS;
  const dim3 grid((unsigned)(blocks < gsl::BATCH_INFO_MAX_BLOCKS ? blocks : gsl::BATCH_INFO_MAX_BLOCKS), n_poses);
  for (int k = 0; k < max_steps; ++k) {
    hipLaunchKernelGGL(gsl::k_map_batch_zero, dim3(1), dim3(gsl::BATCH_ZERO_THREADS), 0, st, (const double*)state,
                       n_poses, (long long*)sums);
    GSL_CHECK_LAUNCH();
    if (photo) {
      hipLaunchKernelGGL(gsl::k_map_batch_photo_info, grid, dim3(gsl::BATCH_INFO_THREADS), 0, st, means,
                         (long long)n_rows, (const float*)work, (const double*)state, fx, fy, cx, cy, depth, width,
                         (float)(width - 2), (float)(height - 2), keep, beyond, kappa, near_plane,
                         (unsigned long long*)sums, photo->colors, photo->intensity, photo->scale,
                         photo->max_residual);
    } else {
      hipLaunchKernelGGL(gsl::k_map_batch_info, grid, dim3(gsl::BATCH_INFO_THREADS), 0, st, means, (long long)n_rows,
                         (const float*)work, (const double*)state, fx, fy, cx, cy, depth, width, (float)(width - 2),
                         (float)(height - 2), keep, beyond, kappa, near_plane, (unsigned long long*)sums);
    }
    GSL_CHECK_LAUNCH();
    hipLaunchKernelGGL(gsl::k_map_batch_step, dim3(1), dim3(gsl::ALIGN_THREADS), 0, st, (const long long*)sums, n_poses,
                       k, max_steps, damping, (long long)min_used, max_rot, max_trans, eps_rot, eps_trans, work,
                       (double*)state, (long long*)history);
    GSL_CHECK_LAUNCH();
  }
  return GSL_OK;
}

extern "C" int gsl_map_pose_align_batch(const float* means, int64_t n_rows, const float* w2c, int n_poses, float fx,
                                        float fy, float cx, float cy, const float* depth, int width, int height,
                                        float keep, float beyond, float kappa, float near_plane, int max_steps,
                                        double damping, int min_used, double max_rot, double max_trans, double eps_rot,
                                        double eps_trans, int64_t* sums, float* work, void* state, void* history,
                                        void* stream) {
  if (!w2c || !sums || !work || !state || !history) return GSL_ERR_BAD_ARG;
  if (n_poses < 1 || n_poses > GSL_MAP_ALIGN_BATCH_MAX_POSES) return GSL_ERR_BAD_ARG;
  if (!gsl::align_args_ok(means, n_rows, fx, fy, cx, cy, depth, width, height, keep, beyond, kappa, max_steps, damping,
                          min_used, max_rot, max_trans, eps_rot, eps_trans))
    return GSL_ERR_BAD_ARG;
  return map_pose_align_batch_run(means, n_rows, w2c, n_poses, fx, fy, cx, cy, depth, width, height, keep, beyond, kappa,
                                  near_plane, max_steps, damping, min_used, max_rot, max_trans, eps_rot, eps_trans, sums,
                                  work, state, history, nullptr, (hipStream_t)stream);
}

extern "C" int gsl_map_pose_align_batch_photo(const float* means, int64_t n_rows, const float* w2c, int n_poses, float fx,
                                              float fy, float cx, float cy, const float* depth, int width, int height,
                                              float keep, float beyond, float kappa, float near_plane, int max_steps,
                                              double damping, int min_used, double max_rot, double max_trans,
                                              double eps_rot, double eps_trans, int64_t* sums, float* work, void* state,
                                              void* history, const float* colors, const float* intensity,
                                              float photo_scale, float photo_max_residual, void* stream) {
  if (!w2c || !sums || !work || !state || !history) return GSL_ERR_BAD_ARG;
  if (n_poses < 1 || n_poses > GSL_MAP_ALIGN_BATCH_MAX_POSES) return GSL_ERR_BAD_ARG;
  if (!gsl::align_args_ok(means, n_rows, fx, fy, cx, cy, depth, width, height, keep, beyond, kappa, max_steps, damping,
                          min_used, max_rot, max_trans, eps_rot, eps_trans))
    return GSL_ERR_BAD_ARG;
  const gsl::InfoPhoto photo = {colors, intensity, photo_scale, photo_max_residual};
  if (!gsl::info_photo_args_ok(photo)) return GSL_ERR_BAD_ARG;
  if (n_rows > gsl_map_info_photo_max_rows(fx, fy, cx, cy, width, height, keep, photo_scale, photo_max_residual))
    return GSL_ERR_BAD_ARG;  // a sum could overflow
  return map_pose_align_batch_run(means, n_rows, w2c, n_poses, fx, fy, cx, cy, depth, width, height, keep, beyond, kappa,
                                  near_plane, max_steps, damping, min_used, max_rot, max_trans, eps_rot, eps_trans, sums,
                                  work, state, history, &photo, (hipStream_t)stream);
}
