// Frame-to-map localisation: a photometric term in the normal equations of a pose (gsplatloc_amd/mapping.py:
// GaussianMap.intensity and the intensity= argument of pose_information, align_pose, align_poses, loop_constraint).
// The point-to-plane sums of map_info.hip use nothing but depth: a frame that sees one wall leaves three moves of the
// camera open.  The map keeps a colour per row, the frame has an image: a row whose intensity differs from the image's at
// its own pixel gives one more equation in the same six parameters, and it is added into the same 30 sums -- the step
// kernels, the batched alignment and everything on the host read them as before.
//
// The intensity image, k_map_photo_intensity, one thread per pixel, once per frame: rgb[height,width,3] float32 in
// 0 .. 255,   Y[v,u] = ((0.299f R + 0.587f G) + 0.114f B) / 255.f.
//
// Per row, where its geometric equation exists and only there (``used`` of map_info.hip, with its predicates
// untouched): p = (x, y, z) its camera point, u, v its unrounded and uf, vf its rounded pixel (map_dev.h), c its colour
// (colors[n,3], 0 .. 1 as k_map_append stores it), s = photo_scale [m per unit of intensity: how many metres of depth
// residual one unit of intensity residual is worth], in float32 with one rounding per operation in the order written:
//   Yi = (0.299f c.r + 0.587f c.g) + 0.114f c.b;
//   Y0, Yl, Yr, Yu, Yd = Y[vf, uf], Y[vf, uf - 1], Y[vf, uf + 1], Y[vf - 1, uf], Y[vf + 1, uf];
//   all six of them t >= 0 and t <= 1 (false for a NaN);
//   gx = (Yr - Yl) * 0.5f,  gy = (Yd - Yu) * 0.5f;
//   Yp = (Y0 + gx * (u - uf)) + gy * (v - vf);   rc = Yp - Yi;   |rc| <= photo_max_residual (beyond it an occluder, a
//     highlight or a wrong row, not a pose error);
//   a0 = (s * gx) * fx / z,  a1 = (s * gy) * fy / z,  a2 = -((a0 * x + a1 * y) / z) -- s times the derivative of Yp by p:
//     u = fx x / z + cx moves by (fx / z, 0, -fx x / z^2) with p;
//   every |a_k| <= 8 (INFO_PHOTO_MAX_A) and z < 16 (INFO_PHOTO_MAX_DEPTH): what bounds the sums, below;
//   Jc = (y a2 - z a1, z a0 - x a2, x a1 - y a0, a0, a1, a2) = (p x a, a),  Jc_6 = s * rc.
// The 28 fix(Jc_a, Jc_b) go into the accumulators of the geometric fix(J_a, J_b): out[0 .. 27] hold geometry plus colour,
// out[28] (used) and out[29] (tested) keep their meaning.  Comparisons false for a NaN, correctly rounded division, no
// contraction: tests/map_photo_ref.py gives the same integers from numpy.  gsl_map_pose_info_photo also fills
// extra[2] int64: the rows that gave a photometric equation, and the sum of fix(s rc, s rc) over them (the colour share
// of out[27]); the alignment entry points pass no extra.  photo_scale = 0 makes every Jc zero: the sums are the
// geometric ones.
//
// No sum can overflow.  With S of map_info.hip (|p| <= z S for a row on an inner pixel), A = 8 and z < 16:
// |a_k| <= A, |(p x a)_k| <= |p| |a| <= 16 S A sqrt(3), |s rc| <= s photo_max_residual, so every |Jc_a| is at most
// Bc = max(16 S A sqrt(3), s photo_max_residual) and a photometric term at most Bc^2 2^20 + 1 in size.  A row adds at
// most one geometric term (B^2 2^20 + 1, map_info.hip) and one photometric term to a sum: n rows stay inside int64 while
// n (1.01^2 (B^2 + Bc^2) 2^20 + 2) < 2^63, the 1 % on B and Bc paying for the float32 roundings as it does there.  That
// n, 2^31 - 1 at the most, is gsl_map_info_photo_max_rows, and the entry points refuse more rows; it is never above
// gsl_map_info_max_rows.  With A = 8 and 16 m (Replica intrinsics at 640 x 480, keep = 0.95, s = 16, residual 1):
// S = 1.20, B = 159, Bc = 266, about 8.9e7 rows -- 70 times the 4 x 640 x 480 a map of that camera is asked to take.
//
// k_map_pose_info_photo is k_map_pose_info with PHOTO set in info_sum_rows (map_info_dev.h, the one copy), the same
// grid.  A used lane reads its colour with one more global_load_dwordx3 and gathers five intensities beside the five
// depths; the second pass of 28 fix goes into the same 56 accumulator registers, the colour share of slot 27 into two
// more.  No float atomics; out and extra are zeroed by launches of zero_u32 in front (never a memset node).
#include "gsloc_internal.h"
#include "map_info_dev.h"

namespace gsl {

constexpr int PHOTO_THREADS = 256;
constexpr int PHOTO_MAX_BLOCKS = 1024;  // k_map_pose_info's grid
constexpr int INTENSITY_THREADS = 256;

__global__ __launch_bounds__(INTENSITY_THREADS) void k_map_photo_intensity(const float* __restrict__ rgb, long long n_px,
                                                                            float* __restrict__ out) {
#pragma clang fp contract(off)
  const long long g = (long long)blockIdx.x * INTENSITY_THREADS + threadIdx.x;
  if (g >= n_px) return;
  const float3 c = map_load_row(rgb, g);
  out[g] = ((0.299f * c.x + 0.587f * c.y) + 0.114f * c.z) / 255.f;
}

__global__ __launch_bounds__(PHOTO_THREADS) void k_map_pose_info_photo(
    const float* __restrict__ means, long long n_rows, const float* __restrict__ w2c, float fx, float fy, float cx,
    float cy, const float* __restrict__ depth, int width, float u_inner, float v_inner, float keep, float beyond,
    float kappa, float near_plane, unsigned long long* __restrict__ out, const float* __restrict__ colors,
    const float* __restrict__ intensity, float photo_scale, float photo_max_residual,
    unsigned long long* __restrict__ extra) {
#pragma clang fp contract(off)
  info_sum_rows<PHOTO_THREADS, true>(means, n_rows, w2c, fx, fy, cx, cy, depth, width, u_inner, v_inner, keep, beyond,
                                     kappa, near_plane, out, colors, intensity, photo_scale, photo_max_residual, extra);
}

// map_pose_info_launch (map_info.hip) with the photometric kernel in place of the geometric one, for arguments that
// gsl_map_pose_info_photo has checked; extra NULL (an iteration of the alignment) or the two words, zeroed here.
int map_pose_info_photo_launch(const float* means, int64_t n_rows, const float* w2c, float fx, float fy, float cx,
                               float cy, const float* depth, int width, int height, float keep, float beyond,
                               float kappa, float near_plane, int64_t* out, const InfoPhoto& photo, int64_t* extra,
                               hipStream_t st) {
  int rc = zero_u32(out, (size_t)2 * GSL_MAP_INFO_VALUES, st);
  if (rc != GSL_OK) return rc;
  if (extra) {
    rc = zero_u32(extra, 4, st);
    if (rc != GSL_OK) return rc;
  }
  const long long blocks = (n_rows + PHOTO_THREADS - 1) / PHOTO_THREADS;
  const int nb = (int)(blocks < PHOTO_MAX_BLOCKS ? blocks : PHOTO_MAX_BLOCKS);
  hipLaunchKernelGGL(k_map_pose_info_photo, dim3(nb), dim3(PHOTO_THREADS), 0, st, means, (long long)n_rows, w2c, fx, fy,
                     cx, cy, depth, width, (float)(width - 2), (float)(height - 2), keep, beyond, kappa, near_plane,
                     (unsigned long long*)out, photo.colors, photo.intensity, photo.scale, photo.max_residual,
                     (unsigned long long*)extra);
  GSL_CHECK_LAUNCH();
  return GSL_OK;
}

}  // namespace gsl

extern "C" int gsl_map_photo_intensity(const float* rgb, int width, int height, float* intensity, void* stream) {
  if (!rgb || !intensity || !gsl::map_image_ok(width, height)) return GSL_ERR_BAD_ARG;
  const long long n_px = (long long)width * height;
  hipLaunchKernelGGL(gsl::k_map_photo_intensity,
                     dim3((unsigned)((n_px + gsl::INTENSITY_THREADS - 1) / gsl::INTENSITY_THREADS)),
                     dim3(gsl::INTENSITY_THREADS), 0, (hipStream_t)stream, rgb, n_px, intensity);
  GSL_CHECK_LAUNCH();
  return GSL_OK;
}

extern "C" int64_t gsl_map_info_photo_max_rows(float fx, float fy, float cx, float cy, int width, int height, float keep,
                                               float photo_scale, float photo_max_residual) {
  if (!gsl::map_image_ok(width, height) || !gsl::map_focal_ok(fx, fy) || !(keep > 0.f && keep <= 1.f)) return 0;
  if (!(photo_scale >= 0.f && photo_scale <= gsl::INFO_PHOTO_MAX_SCALE)) return 0;
  if (!(photo_max_residual >= 0.f && photo_max_residual <= 1.f)) return 0;
  const double ax = fabs(0.5 - (double)cx), bx = fabs((double)width - 1.5 - (double)cx);
  const double ay = fabs(0.5 - (double)cy), by = fabs((double)height - 1.5 - (double)cy);
  const double tx = (ax > bx ? ax : bx) / fabs((double)fx), ty = (ay > by ? ay : by) / fabs((double)fy);
  const double S = sqrt(1.0 + tx * tx + ty * ty);
  const double B = 1.01 * (double)gsl::INFO_MAX_DEPTH * S * (1.0 + 1.0 / (double)keep);
  const double rot = (double)gsl::INFO_PHOTO_MAX_DEPTH * S * (double)gsl::INFO_PHOTO_MAX_A * sqrt(3.0);
  const double res = (double)photo_scale * (double)photo_max_residual;
  const double Bc = 1.01 * (rot > res ? rot : res);
  const double rows = 9223372036854775807.0 / ((B * B + Bc * Bc) * (double)gsl::INFO_ONE + 2.0);
  if (!(rows >= 1.0)) return 0;  // also a NaN: cx, cy not finite
  return rows < 2147483647.0 ? (int64_t)rows : (int64_t)0x7fffffffll;
}

extern "C" int gsl_map_pose_info_photo(const float* means, int64_t n_rows, const float* w2c, float fx, float fy, float cx,
                                       float cy, const float* depth, int width, int height, float keep, float beyond,
                                       float kappa, float near_plane, int64_t* out, const float* colors,
                                       const float* intensity, float photo_scale, float photo_max_residual,
                                       int64_t* extra, void* stream) {
  if (!means || !w2c || !depth || !out || !extra) return GSL_ERR_BAD_ARG;
  if (!gsl::map_rows_ok(n_rows)) return GSL_ERR_BAD_ARG;
  if (!gsl::map_image_ok(width, height) || !gsl::map_focal_ok(fx, fy)) return GSL_ERR_BAD_ARG;
  if (!(keep > 0.f && keep <= 1.f) || !(beyond >= 1.f && beyond < INFINITY)) return GSL_ERR_BAD_ARG;
  if (!(kappa >= 0.f && kappa < INFINITY)) return GSL_ERR_BAD_ARG;
  const gsl::InfoPhoto photo = {colors, intensity, photo_scale, photo_max_residual};
  if (!gsl::info_photo_args_ok(photo)) return GSL_ERR_BAD_ARG;
  if (n_rows > gsl_map_info_photo_max_rows(fx, fy, cx, cy, width, height, keep, photo_scale, photo_max_residual))
    return GSL_ERR_BAD_ARG;  // a sum could overflow
  return gsl::map_pose_info_photo_launch(means, n_rows, w2c, fx, fy, cx, cy, depth, width, height, keep, beyond, kappa,
                                         near_plane, out, photo, extra, (hipStream_t)stream);
}
