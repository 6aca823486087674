// Frame-to-map localisation: how well a depth frame constrains a pose (gsplatloc_amd/mapping.py: pose_information).
// The rows of the map are world points and the frame is a depth image: a row that agrees with the surface its own pixel
// observes gives one point-to-plane equation in the six parameters of a small move of the camera, and the sum of those
// equations over all live rows -- the 6 x 6 information matrix H, the gradient g and the residual sum -- says which
// moves the frame pins down and which it leaves open.  No render, and nothing is written but the 30 sums.
//
// A left perturbation w2c' = exp(xi^) w2c, xi = (omega [rad], upsilon [m]) in the camera's frame, moves a row's camera
// point p to p + omega x p + upsilon.  Against the plane through q0 with unit normal n the residual is r = n . (p - q0)
// and its derivative J = (p x n, n): H = sum J J^T, g = sum J r, delta = -H^-1 g is the Gauss-Newton step.
//
// Row i of means[n,3], projected through w2c to its camera point p = (x, y, z) and to uf, vf (map_dev.h: the one copy
// of the projection), in float32 with one rounding per operation in the order written here:
//   tested = z > near and 1 <= uf <= width - 2 and 1 <= vf <= height - 2 (an inner pixel: the four neighbours exist)
//            and d0 > 0 and d0 < inf, d0 = depth[vf, uf];
//   lo = d0 * keep, hi = d0 * beyond;
//   used   = tested and z >= lo and z <= hi (map_score's "agree") and z < 64 (INFO_MAX_DEPTH: the bound below)
//            and each of dl, dr, du, dd = depth[vf, uf - 1], [vf, uf + 1], [vf - 1, uf], [vf + 1, uf] has
//              d > 0 and d < inf and d >= lo and d <= hi
//            and planar: i0 = 1 / d0, s0 = i0 + i0, tol = kappa * i0,
//              |(1 / dl + 1 / dr) - s0| <= tol and |(1 / du + 1 / dd) - s0| <= tol
//              (the inverse depth of a plane is linear in the pixel: exact on a plane, violated at a crease)
//            and len > 0 (below);
//   q(u, v, d) = (((float)u - cx) / fx * d, ((float)v - cy) / fy * d, d) -- k_map_append's back-projection;
//   a = q(uf + 1, vf, dr) - q(uf - 1, vf, dl),  b = q(uf, vf + 1, dd) - q(uf, vf - 1, du),
//   c = a x b = (a.y b.z - a.z b.y, a.z b.x - a.x b.z, a.x b.y - a.y b.x),
//   len = sqrtf((c.x c.x + c.y c.y) + c.z c.z),  n = c / len (three divisions; its sign cancels in every sum);
//   e = p - q(uf, vf, d0),  r = (n.x e.x + n.y e.y) + n.z e.z,
//   m = p x n = (y n.z - z n.y, z n.x - x n.z, x n.y - y n.x),  J = (m.x, m.y, m.z, n.x, n.y, n.z).
// Comparisons that are false for a NaN; correctly rounded division and sqrtf; no contraction.
//
// The sums are fixed point: fix(s, t) = llrintf((s * t) * 2^20) -- one float32 product, an exact scaling, round half to
// even -- added as int64.  out[30] int64: the 21 fix(J_a, J_b), a <= b, the upper triangle row-major; the 6
// fix(J_a, r); fix(r, r); rows used; rows tested.  Integer sums do not depend on the order of rows, waves or
// workgroups, and the numpy mirror of the tests (tests/map_info_ref.py) gives the same 30 integers.
//
// No sum can overflow.  With tx = max(|0.5 - cx|, |width - 1.5 - cx|) / |fx| and ty likewise -- the tangents of the
// half-angles of the inner pixels, which hold u and v within half a pixel of uf and vf -- and S = sqrt(1 + tx^2 + ty^2):
// a used row has z < 64, so |p| <= 64 S; its pixel's point has d0 <= z / keep, so |q0| <= 64 S / keep; |n| = 1.  Hence
// |n_a| <= 1, |m_a| <= |p| <= 64 S and |r| <= |p - q0| <= 64 S (1 + 1 / keep) =: B, every product is at most B^2 and
// every term at most B^2 2^20 + 1 in size.  n rows stay inside int64 while n (1.01^2 B^2 2^20 + 1) < 2^63 (the 1 % on B
// pays for the float32 roundings of u, n and e): that n, and 2^31 - 1 at the most, is gsl_map_info_max_rows, and the
// entry point refuses more rows.  (Replica intrinsics at 160 x 120, keep = 0.95: about 1.9e8 rows.)
//
// One thread per row over a grid-stride loop, at most INFO_MAX_BLOCKS workgroups.  A thread loads its row once (12 B),
// the lanes that pass the float tests gather five depths.  A lane keeps the 28 sums in 56 registers over all its trips;
// the two counts are ballots and population counts in scalar registers.  After the rows each wave adds its lanes' sums
// (six xor-shuffle steps per value), lane 0 adds them to a table of 30 in LDS (ds_add_u64; 240 B), and the workgroup
// adds its non-zero entries to out with one 64-bit integer atomic each: at most INFO_MAX_BLOCKS x 30 global atomics
// whatever n_rows is.  No float atomics.  out is zeroed by a launch of zero_u32 in front (never a memset node).
//
// All of that, from map_project_point(...) to the atomics on out, is info_sum_rows of map_info_dev.h: the one copy, which
// the batched alignment (map_align_batch.hip) runs for several poses in one launch.
#include "gsloc_internal.h"
#include "map_info_dev.h"

namespace gsl {

constexpr int INFO_THREADS = 256;
constexpr int INFO_MAX_BLOCKS = 1024;  // four workgroups of 256 threads for each of the 256 CUs

__global__ __launch_bounds__(INFO_THREADS) void k_map_pose_info(
    const float* __restrict__ means, long long n_rows, const float* __restrict__ w2c, float fx, float fy, float cx,
    float cy, const float* __restrict__ depth, int width, float u_inner, float v_inner, float keep, float beyond,
    float kappa, float near_plane, unsigned long long* __restrict__ out) {
#pragma clang fp contract(off)
  info_sum_rows<INFO_THREADS, false>(means, n_rows, w2c, fx, fy, cx, cy, depth, width, u_inner, v_inner, keep, beyond,
                                     kappa, near_plane, out, nullptr, nullptr, 0.f, 0.f, nullptr);
}

// The zeroing of out and the launch of k_map_pose_info, for arguments that gsl_map_pose_info has checked: its own two
// launches, and one iteration's of gsl_map_pose_align (map_align.hip), which gives the working pose on the device as w2c.
int map_pose_info_launch(const float* means, int64_t n_rows, const float* w2c, float fx, float fy, float cx, float cy,
                         const float* depth, int width, int height, float keep, float beyond, float kappa,
                         float near_plane, int64_t* out, hipStream_t st) {
  const int rc = zero_u32(out, (size_t)2 * GSL_MAP_INFO_VALUES, st);
  if (rc != GSL_OK) return rc;
  const long long blocks = (n_rows + INFO_THREADS - 1) / INFO_THREADS;
  const int nb = (int)(blocks < INFO_MAX_BLOCKS ? blocks : INFO_MAX_BLOCKS);
  hipLaunchKernelGGL(k_map_pose_info, dim3(nb), dim3(INFO_THREADS), 0, st, means, (long long)n_rows, w2c, fx, fy, cx, cy,
                     depth, width, (float)(width - 2), (float)(height - 2), keep, beyond, kappa, near_plane,
                     (unsigned long long*)out);
  GSL_CHECK_LAUNCH();
  return GSL_OK;
}

}  // namespace gsl

extern "C" int gsl_map_info_values(void) { return GSL_MAP_INFO_VALUES; }

extern "C" int64_t gsl_map_info_max_rows(float fx, float fy, float cx, float cy, int width, int height, float keep) {
  if (!gsl::map_image_ok(width, height) || !gsl::map_focal_ok(fx, fy) || !(keep > 0.f && keep <= 1.f)) return 0;
  const double ax = fabs(0.5 - (double)cx), bx = fabs((double)width - 1.5 - (double)cx);
  const double ay = fabs(0.5 - (double)cy), by = fabs((double)height - 1.5 - (double)cy);
  const double tx = (ax > bx ? ax : bx) / fabs((double)fx), ty = (ay > by ? ay : by) / fabs((double)fy);
  const double B = 1.01 * (double)gsl::INFO_MAX_DEPTH * sqrt(1.0 + tx * tx + ty * ty) * (1.0 + 1.0 / (double)keep);
  const double rows = 9223372036854775807.0 / (B * B * (double)gsl::INFO_ONE + 1.0);
  if (!(rows >= 1.0)) return 0;  // also a NaN: cx, cy not finite
  return rows < 2147483647.0 ? (int64_t)rows : (int64_t)0x7fffffffll;
}

extern "C" int gsl_map_pose_info(const float* means, int64_t n_rows, const float* w2c, float fx, float fy, float cx,
                                 float cy, const float* depth, int width, int height, float keep, float beyond,
                                 float kappa, float near_plane, int64_t* out, void* stream) {
  if (!means || !w2c || !depth || !out) return GSL_ERR_BAD_ARG;
  if (!gsl::map_rows_ok(n_rows)) return GSL_ERR_BAD_ARG;
  if (!gsl::map_image_ok(width, height) || !gsl::map_focal_ok(fx, fy)) return GSL_ERR_BAD_ARG;
  if (!(keep > 0.f && keep <= 1.f) || !(beyond >= 1.f && beyond < INFINITY)) return GSL_ERR_BAD_ARG;
  if (!(kappa >= 0.f && kappa < INFINITY)) return GSL_ERR_BAD_ARG;
  if (n_rows > gsl_map_info_max_rows(fx, fy, cx, cy, width, height, keep)) return GSL_ERR_BAD_ARG;  // a sum could overflow
  return gsl::map_pose_info_launch(means, n_rows, w2c, fx, fy, cx, cy, depth, width, height, keep, beyond, kappa,
                                   near_plane, out, (hipStream_t)stream);
}
