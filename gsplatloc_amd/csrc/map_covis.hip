// Frame-to-map localisation: the covisibility of a depth frame with every frame that built the map
// (gsplatloc_amd/mapping.py: covisibility).  score_poses (map_score.hip) says how many rows of the whole map, or of one
// prefix of it, a frame tests, confirms and sees through from a pose; every row carries the index of the frame that
// appended it (origins, map_correct.hip), so one launch can bin the same three verdicts by that frame: which past frames'
// rows the current frame sees, and whether they agree with it -- what picks the anchor of a loop edge (localizer.py), a
// keyframe to cull, a local map by covisible frames.  No render.
//
// Row i of means[n,3] with o = origins[i], one pose w2c -- the origin is looked at first, as in k_map_correct:
//   outside = o < 0 or o >= n_frames: the row adds one to outside[0] and nothing else, whatever its mean is;
//   otherwise the verdicts of k_map_score for one pose, operation for operation (map_dev.h: the projection and the
//   inside rule):
//   tested = z > near and inside and d > 0 and d < inf, d = depth[vf, uf] -- the row's own pixel, no window;
//   front  = tested and z < d * keep;  behind = tested and z > d * beyond -- one rounded product each;
//   agree  = tested and not front and not behind;
//   counts[o] += (tested, agree, front).
// Comparisons that are false for a NaN.  The sums are integers: they do not depend on the order of rows, waves or
// workgroups, and the numpy mirror of the tests (tests/map_covis_ref.py) gives the same numbers.
//
// One thread per row over a grid-stride loop, at most COVIS_MAX_BLOCKS workgroups; the pose's twelve entries are read
// with a wave-uniform index.  The rows of a map are non-decreasing in origin, so the 64 rows of a wave hold a few runs of
// equal origins -- which is used for speed only: a wave loops over the DISTINCT origins among its tested lanes, whatever
// their order.  It takes the origin of the lowest remaining lane (readlane), ballots origin == o and takes three
// population counts, which lane 0 adds: 64 distinct origins are 64 trips of that loop, shuffled origins cost time and
// nothing else.  One integer atomic per run and non-zero predicate, none per row, no float atomics.
// Where lane 0 adds them: the waves of a workgroup are combined in LDS over a WINDOW of COVIS_WINDOW = 64 consecutive
// origins, [w, w + 64) with w the origin of the first row of the workgroup's trip (every thread reads that one word: the
// decision is the workgroup's) -- a table of 64 x 3 words, 768 B, as k_map_score's.  A run whose origin lies in the
// window is added there (ds_add_u32).  A run whose origin lies OUTSIDE the window -- shuffled origins, a map whose 256
// consecutive rows span more than 64 frames, a first row whose own origin is outside the table -- is added to counts
// directly, with global atomics: the slower path, the same sums.  The window stays while the first row of the next trip
// lies in it (one frame for everything: one flush per workgroup, as k_map_score); when it does not, the workgroup adds
// the table's non-zero entries to counts (one global atomic each), clears it and moves the window, between two
// barriers; after the last trip it adds what is left.  Without the window -- a wave keeping its current run in registers
// across trips and adding it with global atomics -- the kernel took 56 us at 460 800 rows over 48 frames and 142 us
// with one frame for everything, against 15 us of k_map_score on the same rows: 43 000 atomics on five cache lines
// (NOTES.md, "Loops closed in track()", has both).  The rows outside the table are counted as k_map_correct counts
// them: per wave in a register, per workgroup in one word of LDS, one 64-bit atomic per workgroup.  counts and outside
// are zeroed by launches of zero_u32 in front (never a memset node: misc.hip).
#include "gsloc_internal.h"
#include "map_dev.h"

namespace gsl {

constexpr int COVIS_THREADS = 256;
constexpr int COVIS_MAX_BLOCKS = 1024;  // four workgroups of 256 threads for each of the 256 CUs, as k_map_score
constexpr int COVIS_WINDOW = 64;        // consecutive origins whose counts a workgroup combines in LDS
static_assert(3 * COVIS_WINDOW <= COVIS_THREADS, "one thread per entry of the table flushes it");

// The workgroup adds the non-zero entries of its table to counts and clears them; between two barriers of the caller.
// An entry is non-zero only where a tested row had the origin win + j -- the 32-bit sum, which wraps as the slot's
// difference did when win came from a row whose own origin is negative -- and that origin is inside counts.
__device__ static inline void covis_flush(uint32_t* table, int32_t* __restrict__ counts, uint32_t win) {
  if ((int)threadIdx.x < 3 * COVIS_WINDOW) {
    const uint32_t c = table[threadIdx.x];
    if (c != 0u) {
      const uint32_t o = win + threadIdx.x / 3u;  // modulo 2^32, on purpose
      atomicAdd(&counts[3 * (size_t)o + threadIdx.x % 3u], (int32_t)c);
      table[threadIdx.x] = 0u;
    }
  }
}

__global__ __launch_bounds__(COVIS_THREADS) void k_map_covis(
    const float* __restrict__ means, const int32_t* __restrict__ origins, long long n_rows,
    const float* __restrict__ w2c, float fx, float fy, float cx, float cy, const float* __restrict__ depth, int width,
    float u_last, float v_last, float keep, float beyond, float near_plane, int n_frames, int32_t* __restrict__ counts,
    unsigned long long* __restrict__ outside_rows) {
  __shared__ uint32_t table[3 * COVIS_WINDOW];
  __shared__ uint32_t block_outside;
  if ((int)threadIdx.x < 3 * COVIS_WINDOW) table[threadIdx.x] = 0u;
  if (threadIdx.x == 0) block_outside = 0u;
  __syncthreads();
  const bool first_lane = (threadIdx.x & 63) == 0;
  uint32_t wave_outside = 0;
  const long long first_base = (long long)blockIdx.x * COVIS_THREADS;  // below n_rows: the grid has no idle workgroup
  uint32_t win = (uint32_t)origins[first_base];  // the window's first origin (unsigned: an origin may be anything)
  const long long stride = (long long)gridDim.x * COVIS_THREADS;
  // the trip count is the workgroup's: every lane of a wave reaches every ballot, every wave every barrier
  for (long long base = first_base; base < n_rows; base += stride) {
    const uint32_t first = (uint32_t)origins[base];  // one word for the whole workgroup
    if (first - win >= (uint32_t)COVIS_WINDOW) {     // ... and so is this decision
      __syncthreads();
      covis_flush(table, counts, win);
      __syncthreads();
      win = first;
    }
    const long long g = base + threadIdx.x;
    int o = -1;
    bool outside = false, tested = false, front = false, behind = false;
    if (g < n_rows) {
      o = origins[g];
      outside = o < 0 || o >= n_frames;
      if (!outside) {
        const MapPixel p = map_project(w2c, map_load_row(means, g), fx, fy, cx, cy);
        tested = p.z > near_plane && map_inside(p, u_last, v_last);
        if (tested) {  // the index is inside
          const float d = depth[(size_t)(int)p.vf * (size_t)width + (size_t)(int)p.uf];
          tested = d > 0.f && d < INFINITY;
          front = tested && p.z < d * keep;
          behind = tested && p.z > d * beyond;
        }
      }
    }
    const bool agree = tested && !front && !behind;
    wave_outside += (uint32_t)__popcll(__ballot(outside));
    const unsigned long long b_agree = __ballot(agree), b_front = __ballot(front);
    unsigned long long rest = __ballot(tested);  // wave-uniform: so is the loop
    while (rest != 0ull) {
      const int run_o = __builtin_amdgcn_readlane(o, __ffsll((long long)rest) - 1);  // the lowest remaining lane's
      const unsigned long long run = __ballot(tested && o == run_o);                 // ... which is in it
      if (first_lane) {  // run_o is inside counts: it came from a tested lane
        const uint32_t n_tested = (uint32_t)__popcll(run), n_agree = (uint32_t)__popcll(run & b_agree),
                       n_front = (uint32_t)__popcll(run & b_front);
        const uint32_t slot = (uint32_t)run_o - win;
        if (slot < (uint32_t)COVIS_WINDOW) {
          atomicAdd(&table[3 * slot], n_tested);
          if (n_agree != 0u) atomicAdd(&table[3 * slot + 1], n_agree);
          if (n_front != 0u) atomicAdd(&table[3 * slot + 2], n_front);
        } else {  // outside the window: straight to counts
          int32_t* c = counts + 3 * (size_t)run_o;
          atomicAdd(&c[0], (int32_t)n_tested);
          if (n_agree != 0u) atomicAdd(&c[1], (int32_t)n_agree);
          if (n_front != 0u) atomicAdd(&c[2], (int32_t)n_front);
        }
      }
      rest &= ~run;
    }
  }
  if (first_lane && wave_outside != 0u) atomicAdd(&block_outside, wave_outside);
  __syncthreads();
  covis_flush(table, counts, win);
  if (threadIdx.x == 0 && block_outside != 0u) atomicAdd(outside_rows, (unsigned long long)block_outside);
}

}  // namespace gsl

extern "C" int gsl_map_covis(const float* means, const int32_t* origins, int64_t n_rows, const float* w2c, float fx,
                             float fy, float cx, float cy, const float* depth, int width, int height, float keep,
                             float beyond, float near_plane, int n_frames, int32_t* counts, int64_t* outside,
                             void* stream) {
  if (!means || !origins || !w2c || !depth || !counts || !outside) return GSL_ERR_BAD_ARG;
  if (n_frames < 1 || n_frames > GSL_MAP_COVIS_MAX_FRAMES) return GSL_ERR_BAD_ARG;
  if (!gsl::map_image_ok(width, height) || !gsl::map_focal_ok(fx, fy)) return GSL_ERR_BAD_ARG;
  if (!(keep > 0.f && keep <= 1.f) || !(beyond >= 1.f)) return GSL_ERR_BAD_ARG;
  if (n_rows == 0) return GSL_OK;  // an empty map: nothing to launch, counts and outside are not touched
  if (!gsl::map_rows_ok(n_rows)) return GSL_ERR_BAD_ARG;
  hipStream_t st = (hipStream_t)stream;
  int rc = gsl::zero_u32(counts, (size_t)3 * (size_t)n_frames, st);
  if (rc != GSL_OK) return rc;
  rc = gsl::zero_u32(outside, 2, st);  // one 64-bit word
  if (rc != GSL_OK) return rc;
  const long long blocks = (n_rows + gsl::COVIS_THREADS - 1) / gsl::COVIS_THREADS;
  const int nb = (int)(blocks < gsl::COVIS_MAX_BLOCKS ? blocks : gsl::COVIS_MAX_BLOCKS);
  hipLaunchKernelGGL(gsl::k_map_covis, dim3(nb), dim3(gsl::COVIS_THREADS), 0, st, means, origins, (long long)n_rows, w2c,
                     fx, fy, cx, cy, depth, width, (float)(width - 1), (float)(height - 1), keep, beyond, near_plane,
                     n_frames, counts, (unsigned long long*)outside);
  GSL_CHECK_LAUNCH();
  return GSL_OK;
}
