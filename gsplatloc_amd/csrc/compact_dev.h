// Order-preserving stream compaction, the one copy: of n items, one per thread, those a rule keeps get an output row,
// in ascending item order.  Used by the packed projection (project_packed.hip), map growth (map.hip) and the view
// selection (map_view.hip).  Two passes over the items with a scan in between:
//   record  the kernel evaluates its rule and calls compact_record: a 64-bit ballot per wave, a count per workgroup;
//   scan    launch_count_scan (compact.hip): exclusive scan of the workgroup counts -> bases, total -> a counter;
//   fill    the lanes whose ballot bit is set (compact_kept) produce their row and store it at compact_position:
//           workgroup base + kept lanes of the earlier waves + kept lower lanes of this wave (mbcnt).
// No workgroup waits for another one: no look-back scan and no "last workgroup" ticket (both need device-scope
// release/acquire across the eight XCD L2s, NOTES.md round 3), and no atomics (the order would be run-dependent).
// The fill pass takes its positions from the stored ballots alone, so the two passes cannot disagree about where a row
// goes.
// What the two passes of a user must agree on is here and nowhere else: 256 threads = 4 waves per workgroup, 32-bit
// counts (the callers refuse n >= 2^31), the layout of the workspace.
#pragma once
#include "gsloc_common.h"

namespace gsl {

constexpr int COMPACT_THREADS = 256;  // items per workgroup, one per thread
constexpr int COMPACT_WAVES = COMPACT_THREADS / 64;

static inline long long compact_blocks(long long n) { return (n + COMPACT_THREADS - 1) / COMPACT_THREADS; }

// ws = [ballots nb x 4 uint64][counts nb][bases nb][extra columns, nb each] (uint32); nb = compact_blocks(n), at least 1
struct CompactWs {
  uint64_t* ballots;
  uint32_t *counts, *bases, *extra;
};
static inline size_t compact_ws_bytes(long long n, int extra_u32_columns = 0) {
  const long long nb = n > 0 ? compact_blocks(n) : 1;
  return (size_t)nb * (COMPACT_WAVES * sizeof(uint64_t) + (2 + extra_u32_columns) * sizeof(uint32_t));
}
static inline CompactWs compact_ws(void* ws, int nb) {
  CompactWs w;
  w.ballots = (uint64_t*)ws;
  w.counts = (uint32_t*)(w.ballots + (size_t)nb * COMPACT_WAVES);
  w.bases = w.counts + nb;
  w.extra = w.bases + nb;
  return w;
}

// Counts K wave masks per workgroup: true in the workgroup's thread 0 alone, where sum[k] is then the set bits of
// mask[k] over the four waves (of a wave's mask only lane 0's value is read).  One barrier however many masks; every
// thread of the workgroup calls it.
template <int K>
__device__ static inline bool compact_block_sums(const unsigned long long (&mask)[K], uint32_t (&sum)[K]) {
  __shared__ uint32_t cnt[K][COMPACT_WAVES];
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int k = 0; k < K; ++k) cnt[k][threadIdx.x >> 6] = (uint32_t)__popcll(mask[k]);
  }
  __syncthreads();
  if (threadIdx.x != 0) return false;
  static_assert(COMPACT_WAVES == 4, "the sum over the waves is written out");
#pragma unroll
  for (int k = 0; k < K; ++k) sum[k] = cnt[k][0] + cnt[k][1] + cnt[k][2] + cnt[k][3];
  return true;
}

// Where this thread's wave has its ballot.
__device__ static inline size_t compact_wave_slot() { return (size_t)blockIdx.x * COMPACT_WAVES + (threadIdx.x >> 6); }

// Record step, first half: the wave's ballot of keep -> ballots[compact_wave_slot()]; returns it.
__device__ static inline unsigned long long compact_ballot(bool keep, uint64_t* __restrict__ ballots) {
  const unsigned long long kept = __ballot(keep);
  if ((threadIdx.x & 63) == 0) ballots[compact_wave_slot()] = kept;
  return kept;
}

// Record step: the ballot and the workgroup's count.  Every thread of the workgroup calls it (a barrier inside).
__device__ static inline void compact_record(bool keep, uint64_t* __restrict__ ballots,
                                             uint32_t* __restrict__ block_counts) {
  const unsigned long long mask[1] = {compact_ballot(keep, ballots)};
  uint32_t sum[1];
  if (compact_block_sums(mask, sum)) block_counts[blockIdx.x] = sum[0];
}

// Fill pass: whether the record pass kept this thread's item.
__device__ static inline bool compact_kept(const uint64_t* __restrict__ ballots) {
  return (ballots[compact_wave_slot()] >> (threadIdx.x & 63)) & 1ull;
}

// Position step: the output row of this thread's item, if it was kept: the rows of earlier workgroups, of earlier waves
// of this one, of lower lanes of this wave.
__device__ static inline long long compact_position(const uint64_t* __restrict__ ballots,
                                                    const uint32_t* __restrict__ block_bases) {
  const int wv = threadIdx.x >> 6;
  const uint64_t* mine = ballots + (size_t)blockIdx.x * COMPACT_WAVES;
  const unsigned long long kept = mine[wv];
  long long pos = block_bases[blockIdx.x];
  for (int w = 0; w < wv; ++w) pos += __popcll(mine[w]);
  return pos + __builtin_amdgcn_mbcnt_hi((uint32_t)(kept >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)kept, 0u));
}

// Fill pass, the grid's first thread: stored[0] = min(total[0], room), the rows that the fill pass writes.
__device__ static inline void compact_store_clamped(const int32_t* total, long long room, int32_t* stored) {
  if ((long long)blockIdx.x * COMPACT_THREADS + threadIdx.x == 0) {
    const long long t = total[0];
    stored[0] = (int32_t)(t < room ? t : room);
  }
}

}  // namespace gsl
