// Frame-to-map localisation: how well a depth frame, seen from each of K candidate poses, agrees with the map
// (gsplatloc_amd/mapping.py: score_poses).  The rows of the map are world points and the frame is a depth image: a
// row that projects into the image lies in front of, at or behind the surface its own pixel observes, and the counts of
// those verdicts over all live rows say whether a pose can be the frame's -- the acceptance test of an estimate and the
// choice among the candidate starts of a relocalisation (gsplatloc_amd/localizer.py).  No render.
//
// Row i of means[n,3], pose k, projected through w2c[k] to z, uf, vf (map_dev.h: the projection and the inside rule):
//   tested = z > near and inside and d > 0 and d < inf, d = depth[vf, uf] -- the row's own pixel, no window;
//   front  = tested and z < d * keep;  behind = tested and z > d * beyond -- one rounded product each;
//   agree  = tested and not front and not behind;
//   counts[k] = (rows tested, rows that agree, rows in front).
// Comparisons that are false for a NaN: NaN / inf rows, rows behind the camera or outside the image and pixels without
// depth add nothing, a row with z == d * keep or z == d * beyond agrees.  The sums are integers: they do not depend on
// the order of rows, waves or workgroups, and the numpy mirror of the tests gives the same three numbers.
//
// One thread per row over a grid-stride loop, at most SCORE_MAX_BLOCKS workgroups.  A thread loads its row once (12 B)
// and loops over the poses; a pose's twelve entries are read with a wave-uniform index (scalar loads through the
// constant cache), so a pose costs a lane 18 multiply-adds, two divisions and -- for the lanes that passed the float
// tests only -- one depth gather.  Per pose and predicate one ballot and one population count per wave, which lane 0
// adds to a table [n_poses][3] in LDS (ds_add_u32; 768 B); after the rows the workgroup adds its non-zero entries to
// counts with one integer atomic each: at most SCORE_MAX_BLOCKS x 3 x n_poses global atomics whatever n_rows is.  No
// float atomics.  counts is zeroed by a launch of zero_u32 in front (never a memset node: misc.hip).
#include "gsloc_internal.h"
#include "map_dev.h"

namespace gsl {

constexpr int SCORE_THREADS = 256;
constexpr int SCORE_MAX_BLOCKS = 1024;  // four workgroups of 256 threads for each of the 256 CUs
constexpr int SCORE_COUNTS = 3 * GSL_MAP_SCORE_MAX_POSES;
static_assert(SCORE_COUNTS <= SCORE_THREADS, "one thread per entry of the table flushes it");

__global__ __launch_bounds__(SCORE_THREADS) void k_map_score(
    const float* __restrict__ means, long long n_rows, const float* __restrict__ w2c, int n_poses, float fx, float fy,
    float cx, float cy, const float* __restrict__ depth, int width, float u_last, float v_last, float keep, float beyond,
    float near_plane, int32_t* __restrict__ counts) {
  __shared__ uint32_t table[SCORE_COUNTS];
  if ((int)threadIdx.x < SCORE_COUNTS) table[threadIdx.x] = 0u;
  __syncthreads();
  const bool first_lane = (threadIdx.x & 63) == 0;
  const long long stride = (long long)gridDim.x * SCORE_THREADS;
  // the trip count is the workgroup's: every lane of a wave reaches every ballot
  for (long long base = (long long)blockIdx.x * SCORE_THREADS; base < n_rows; base += stride) {
    const long long g = base + threadIdx.x;
    const bool live = g < n_rows;
    float3 row = {0.f, 0.f, 0.f};
    if (live) row = map_load_row(means, g);
    for (int k = 0; k < n_poses; ++k) {
      const MapPixel p = map_project(w2c + 16 * k, row, fx, fy, cx, cy);  // the pose: wave-uniform
      bool tested = live && p.z > near_plane && map_inside(p, u_last, v_last);
      bool front = false, behind = false;
      if (tested) {  // the index is inside
        const float d = depth[(size_t)(int)p.vf * (size_t)width + (size_t)(int)p.uf];
        tested = d > 0.f && d < INFINITY;
        front = tested && p.z < d * keep;
        behind = tested && p.z > d * beyond;
      }
      const bool agree = tested && !front && !behind;
      const unsigned long long b_tested = __ballot(tested), b_agree = __ballot(agree), b_front = __ballot(front);
      if (first_lane && b_tested != 0ull) {
        atomicAdd(&table[3 * k], (uint32_t)__popcll(b_tested));
        if (b_agree != 0ull) atomicAdd(&table[3 * k + 1], (uint32_t)__popcll(b_agree));
        if (b_front != 0ull) atomicAdd(&table[3 * k + 2], (uint32_t)__popcll(b_front));
      }
    }
  }
  __syncthreads();
  if ((int)threadIdx.x < 3 * n_poses) {
    const uint32_t c = table[threadIdx.x];
    if (c != 0u) atomicAdd(&counts[threadIdx.x], (int32_t)c);
  }
}

}  // namespace gsl

extern "C" int gsl_map_score_max_poses(void) { return GSL_MAP_SCORE_MAX_POSES; }

extern "C" int gsl_map_score(const float* means, int64_t n_rows, const float* w2c, int n_poses, float fx, float fy,
                             float cx, float cy, const float* depth, int width, int height, float keep, float beyond,
                             float near_plane, int32_t* counts, void* stream) {
  if (!means || !w2c || !depth || !counts) return GSL_ERR_BAD_ARG;
  if (!gsl::map_rows_ok(n_rows) || n_poses < 1 || n_poses > GSL_MAP_SCORE_MAX_POSES) return GSL_ERR_BAD_ARG;
  if (!gsl::map_image_ok(width, height) || !gsl::map_focal_ok(fx, fy)) return GSL_ERR_BAD_ARG;
  if (!(keep > 0.f && keep <= 1.f) || !(beyond >= 1.f)) return GSL_ERR_BAD_ARG;
  hipStream_t st = (hipStream_t)stream;
  const int rc = gsl::zero_u32(counts, (size_t)3 * (size_t)n_poses, st);
  if (rc != GSL_OK) return rc;
  const long long blocks = (n_rows + gsl::SCORE_THREADS - 1) / gsl::SCORE_THREADS;
  const int nb = (int)(blocks < gsl::SCORE_MAX_BLOCKS ? blocks : gsl::SCORE_MAX_BLOCKS);
  hipLaunchKernelGGL(gsl::k_map_score, dim3(nb), dim3(gsl::SCORE_THREADS), 0, st, means, (long long)n_rows, w2c, n_poses,
                     fx, fy, cx, cy, depth, width, (float)(width - 1), (float)(height - 1), keep, beyond, near_plane,
                     counts);
  GSL_CHECK_LAUNCH();
  return GSL_OK;
}
