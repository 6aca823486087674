// Frame-to-map localisation: the rows follow a corrected trajectory (gsplatloc_amd/mapping.py: correct).  A row is
// written into the world once, at the estimate of the frame that saw it; every row carries the index of that frame
// (origins), and when the trajectory is corrected -- a loop closed, a pose graph solved -- the rows of frame k are moved
// by the rigid transform D_k that took the old pose of frame k to the new one.
//
// gsl_map_correct, one thread per row.  Row i of means[n,3] with o = origins[i], e = table[12 o .. 12 o + 11] the
// row-major 3 x 4 [R | t] of frame o:
//   inside  = 0 <= o < n_frames;
//   moved   = inside and x, y, z finite and e is not the identity -- twelve == comparisons against 1 0 0 0 / 0 1 0 0 /
//             0 0 1 0, so that -0.0 counts as 0 and an entry with a NaN is "not the identity";
//   a moved row becomes  x' = ((e0 x + e1 y) + e2 z) + e3,  y' = ((e4 x + e5 y) + e6 z) + e7,
//             z' = ((e8 x + e9 y) + e10 z) + e11 -- the bracket order of map_project (map_dev.h);
//   every other row keeps every bit: a NaN or inf row, a -0.0 coordinate under an identity entry (which the product
//             would turn into +0.0), an origin outside the table.
// float32, every operation rounded once in the order written (no contraction): on given inputs the rule has no rounding
// freedom, and the numpy mirror of the tests (tests/map_correct_ref.py) gives the same bits.
//
// One thread per row over a grid-stride loop, at most CORRECT_MAX_BLOCKS workgroups.  A thread reads its origin (4 B)
// and its row (12 B, one dwordx3), then its entry (48 B, three dwordx4) and writes its own row in place, which no other
// thread reads: 16 B read and at most 12 B written per row, and a table of 48 B per frame that stays in L2.  The
// origins are non-decreasing in map order, so the lanes of a wave read one or two entries -- the same three or six
// lines -- and the loads coalesce to that; the entry is not fetched once per wave through a scalar path: that needs a
// uniformity test and a second code path for the wave that spans two frames, and at 460 800 rows the kernel's 10 us
// are its dependent loads and its atomics, not its bytes ("Trajectory correction"; NOTES.md has the
// measurement).
// counters[0] = rows moved, counters[1] = rows whose origin is outside the table: one ballot and one population count
// per wave, trip and counter, summed in wave-uniform registers; after the rows lane 0 of every wave adds its sums to two
// words of LDS and the workgroup adds those to the counters with ONE 64-bit integer atomic each -- at most
// CORRECT_MAX_BLOCKS atomics on an address whatever n_rows is (map_refine.hip: why not one per wave).  Integer sums: they
// do not depend on the order.  No LDS beyond the two words, no float atomics.  The counters are zeroed by a launch of
// zero_u32 in front (never a memset node: misc.hip).
#include "compact_dev.h"
#include "gsloc_internal.h"
#include "map_dev.h"

namespace gsl {

constexpr int CORRECT_MAX_BLOCKS = 512;  // two workgroups of 256 threads for each of the 256 CUs

__global__ __launch_bounds__(COMPACT_THREADS) void k_map_correct(
    float* __restrict__ means, const int32_t* __restrict__ origins, long long n_rows,
    const float* __restrict__ table, int n_frames, unsigned long long* __restrict__ counters) {
#pragma clang fp contract(off)
  __shared__ uint32_t block_count[2];
  if (threadIdx.x < 2) block_count[threadIdx.x] = 0u;
  __syncthreads();
  uint32_t wave_moved = 0, wave_outside = 0;
  const long long stride = (long long)gridDim.x * COMPACT_THREADS;
  // the trip count is the workgroup's: every lane of a wave reaches every ballot
  for (long long base = (long long)blockIdx.x * COMPACT_THREADS; base < n_rows; base += stride) {
    const long long g = base + threadIdx.x;
    bool moved = false, outside = false;
    if (g < n_rows) {
      const int o = origins[g];
      outside = o < 0 || o >= n_frames;
      if (!outside) {
        const float3 p = map_load_row(means, g);
        const float* e = table + 12 * (size_t)o;
        const float4 e0 = {e[0], e[1], e[2], e[3]}, e1 = {e[4], e[5], e[6], e[7]}, e2 = {e[8], e[9], e[10], e[11]};
        const bool finite = fabsf(p.x) < INFINITY && fabsf(p.y) < INFINITY && fabsf(p.z) < INFINITY;
        const bool identity = e0.x == 1.f && e0.y == 0.f && e0.z == 0.f && e0.w == 0.f && e1.x == 0.f && e1.y == 1.f &&
                              e1.z == 0.f && e1.w == 0.f && e2.x == 0.f && e2.y == 0.f && e2.z == 1.f && e2.w == 0.f;
        moved = finite && !identity;
        if (moved) {
          const float x = ((e0.x * p.x + e0.y * p.y) + e0.z * p.z) + e0.w;
          const float y = ((e1.x * p.x + e1.y * p.y) + e1.z * p.z) + e1.w;
          const float z = ((e2.x * p.x + e2.y * p.y) + e2.z * p.z) + e2.w;
          map_store_row(means, g, {x, y, z});
        }
      }
    }
    wave_moved += (uint32_t)__popcll(__ballot(moved));
    wave_outside += (uint32_t)__popcll(__ballot(outside));
  }
  if ((threadIdx.x & 63) == 0) {
    if (wave_moved != 0u) atomicAdd(&block_count[0], wave_moved);
    if (wave_outside != 0u) atomicAdd(&block_count[1], wave_outside);
  }
  __syncthreads();
  if (threadIdx.x < 2 && block_count[threadIdx.x] != 0u)
    atomicAdd(&counters[threadIdx.x], (unsigned long long)block_count[threadIdx.x]);
}

}  // namespace gsl

extern "C" int gsl_map_correct(float* means, const int32_t* origins, int64_t n_rows, const float* table, int n_frames,
                               int64_t* counters, void* stream) {
  if (!means || !origins || !table || !counters) return GSL_ERR_BAD_ARG;
  if (n_frames < 1) return GSL_ERR_BAD_ARG;
  if (n_rows == 0) return GSL_OK;  // an empty map: nothing to launch, the counters are not touched
  if (!gsl::map_rows_ok(n_rows)) return GSL_ERR_BAD_ARG;
  hipStream_t st = (hipStream_t)stream;
  const int rc = gsl::zero_u32(counters, 4, st);  // two 64-bit words
  if (rc != GSL_OK) return rc;
  const long long blocks = gsl::compact_blocks(n_rows);
  const int nb = (int)(blocks < gsl::CORRECT_MAX_BLOCKS ? blocks : gsl::CORRECT_MAX_BLOCKS);
  hipLaunchKernelGGL(gsl::k_map_correct, dim3(nb), dim3(gsl::COMPACT_THREADS), 0, st, means, origins,
                     (long long)n_rows, table, n_frames, (unsigned long long*)counters);
  GSL_CHECK_LAUNCH();
  return GSL_OK;
}
