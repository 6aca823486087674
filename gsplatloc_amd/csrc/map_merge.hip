// Frame-to-map localisation: a map with a resolution (gsplatloc_amd/mapping.py: merge).  The live rows that fall into
// the same cube of side h -- the same VOXEL -- become one row, at the voxel's first row in map order, so that the rows
// that stay keep the map's order and the shared ordered compaction (compact_dev.h) carries them.
//
// The rule (include/gsloc_hip.h), per row and axis a:  f_a = p_a * inv_h (one rounded float32 product), c_a = floorf(f_a);
// MERGEABLE when the three f_a are finite and |c_a| <= 2^20 - 1; key = the cells biased by 2^20 - 1, 21 bits each.  Per
// voxel, over its k mergeable rows: first = the smallest row, S_a = sum of q_a = rintf((f_a - c_a) * 65536), C_j = sum of
// rintf(clamp(colour_j, 0, 1) * 65280), T = the largest stamp.  k == 1: the row is untouched.  k > 1: the rows other than
// first are removed, first gets mean_a = (float)((c_a + S_a / (65536 k)) h), colour_j = (float)(C_j / (65280 k)) in
// double, and the stamp T.  Every sum is an integer: the result does not depend on the order in which rows arrive,
// which float atomics could not offer (the map mode is deterministic, and held bit for bit against a numpy mirror).
//
// The launches of gsl_map_merge_select:
//   k_map_merge_clear   every slot of the table: key = all ones (empty), count 0, first = all ones; the flag; h;
//   k_map_merge_insert  a row finds or claims the slot of its key -- open addressing, linear probing from a hash of the
//                       key, ONE 64-bit compare-and-swap per probe -- then count += 1 and first = min(first, row) with
//                       integer atomics, and stores its slot.  What a slot's key is, is known here only from what the
//                       compare-and-swap returned, never from a plain load: the eight XCD L2s are not coherent for plain
//                       loads inside one launch (NOTES.md, round 3).  The loop ends after as many probes as there are
//                       slots at the latest; no thread waits for another.  A row that found no slot (it cannot happen
//                       in a table half empty) is treated as not mergeable and sets the flag, which the host reads with
//                       the counters and raises on;
//   k_map_merge_select  stays = not mergeable or first == own row, recorded in the head of ws in the layout of
//                       gsl_map_view_select; the rows that go are the second count.  The first row of a voxel with
//                       k > 1 clears its own sums -- they are indexed by that row, so only merged voxels pay for them;
//   launch_count_scan   twice: rows that stay -> counters[0], rows removed -> counters[1];
//   k_map_merge_sum     only rows whose slot has count > 1 add q, colour (64-bit integer adds) and stamp (integer max):
//                       a map without duplicates pays the three atomics of the insertion per row and nothing here.
// Then the caller runs gsl_map_view_gather and gsl_map_gather_i32 (unchanged) into the spare buffers, and
//   k_map_merge_apply   one thread per stored row r < counters[2]: where the voxel of its old row ids[r] has k > 1 (that
//                       row is the voxel's first), the mean, the colour and the stamp of the rule overwrite row r.  The
//                       cells come back out of the slot's key, h out of the workspace: a handful of doubles per voxel.
//
// ws = [head: gsl_map_view_ws_bytes(n) -- ballots of the rows that stay nb x 4 uint64, counts nb, bases nb, removed
//       counts nb, their bases nb][params: flag, h (float bits), 0, 0 (uint32)][table: slots x (key uint64, count
//       uint32, first uint32)][sums n x 6 uint64: S_0 S_1 S_2 C_0 C_1 C_2, indexed by a voxel's first row][largest stamps
//       n int32, likewise][slot of every row n uint32, all ones: none];  slots = the smallest power of two >= 2 n.
#include "compact_dev.h"
#include "gsloc_internal.h"
#include "map_dev.h"

namespace gsl {

constexpr uint64_t MERGE_EMPTY = ~0ull;     // no key has bit 63 set
constexpr uint32_t MERGE_NONE = ~0u;        // slot of a row that is not mergeable; first of an empty slot
constexpr int MERGE_CELL_BIAS = (1 << 20) - 1;  // cells -(2^20 - 1) .. 2^20 - 1 -> 0 .. 2^21 - 2
constexpr float MERGE_CELL_MAX = 1048575.f;
constexpr int MERGE_PARAMS = 4;  // flag, h, two spare words (keeps the table 16-byte aligned)

struct MergeSlot {
  unsigned long long key;
  uint32_t count, first;
};
static_assert(sizeof(MergeSlot) == 16, "one dwordx4 per slot");

struct MergeWs {
  CompactWs head;  // extra columns: removed counts, removed bases
  uint32_t* params;
  MergeSlot* table;
  unsigned long long* sums;
  int32_t* tmax;
  uint32_t* slot_of;
  size_t slots;
};
static inline size_t merge_slots(long long n) {
  size_t t = 2;
  while (t < 2 * (size_t)n) t <<= 1;
  return t;
}
static inline size_t merge_ws_bytes(long long n) {
  const long long rows = n > 0 ? n : 1;
  return compact_ws_bytes(n, 2) + MERGE_PARAMS * sizeof(uint32_t) + merge_slots(rows) * sizeof(MergeSlot) +
         (size_t)rows * (6 * sizeof(unsigned long long) + sizeof(int32_t) + sizeof(uint32_t));
}
static inline MergeWs merge_ws(void* ws, long long n, int nb) {
  MergeWs w;
  w.head = compact_ws(ws, nb);
  w.params = (uint32_t*)((char*)ws + compact_ws_bytes(n, 2));  // 48 nb bytes in: aligned for 16
  w.slots = merge_slots(n);
  w.table = (MergeSlot*)(w.params + MERGE_PARAMS);
  w.sums = (unsigned long long*)(w.table + w.slots);
  w.tmax = (int32_t*)(w.sums + 6 * (size_t)n);
  w.slot_of = (uint32_t*)(w.tmax + n);
  return w;
}

// The float32 part of the rule for one row: whether it is mergeable, its key and its three fractions q.
struct MergeCell {
  bool mergeable;
  unsigned long long key;
  uint32_t q[3];
};
__device__ static inline MergeCell merge_cell(const float* __restrict__ means, long long g, float inv_h) {
#pragma clang fp contract(off)
  MergeCell m;
  m.mergeable = true;
  m.key = 0ull;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const float f = means[3 * (size_t)g + a] * inv_h;
    const float c = floorf(f);
    // false for a NaN; an infinite f has an infinite c
    const bool ok = fabsf(f) < INFINITY && fabsf(c) <= MERGE_CELL_MAX;
    m.mergeable = m.mergeable && ok;
    const int cell = ok ? (int)c : 0;
    m.key |= (unsigned long long)(uint32_t)(cell + MERGE_CELL_BIAS) << (21 * a);
    m.q[a] = ok ? (uint32_t)rintf((f - c) * 65536.f) : 0u;
  }
  return m;
}

// Where the probing of a key starts: the finaliser of splitmix64.  Internal: no result depends on it.
__device__ static inline size_t merge_hash(unsigned long long k) {
  k ^= k >> 30;
  k *= 0xbf58476d1ce4e5b9ull;
  k ^= k >> 27;
  k *= 0x94d049bb133111ebull;
  k ^= k >> 31;
  return (size_t)k;
}

__global__ __launch_bounds__(256) void k_map_merge_clear(MergeSlot* __restrict__ table, size_t slots, float h,
                                                        uint32_t* __restrict__ params) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i == 0) {
    params[0] = 0u;  // no row was left without a slot
    params[1] = __float_as_uint(h);
    params[2] = 0u;
    params[3] = 0u;
  }
  if (i >= slots) return;
  MergeSlot s;
  s.key = MERGE_EMPTY;
  s.count = 0u;
  s.first = MERGE_NONE;
  table[i] = s;
}

__global__ __launch_bounds__(COMPACT_THREADS) void k_map_merge_insert(const float* __restrict__ means, long long n_rows,
                                                                     float inv_h, MergeSlot* table, size_t slots,
                                                                     uint32_t* __restrict__ slot_of, uint32_t* flag) {
  const long long g = (long long)blockIdx.x * COMPACT_THREADS + threadIdx.x;
  if (g >= n_rows) return;
  const MergeCell m = merge_cell(means, g, inv_h);
  uint32_t mine = MERGE_NONE;
  if (m.mergeable) {
    const size_t mask = slots - 1;
    size_t s = merge_hash(m.key) & mask;
    for (size_t probe = 0; probe < slots; ++probe) {  // bounded: nothing spins
      if (s == (size_t)MERGE_NONE) s = 0;  // 2^32 slots: the last one would read as "none" and is never used
      const unsigned long long was = atomicCAS(&table[s].key, MERGE_EMPTY, m.key);
      if (was == MERGE_EMPTY || was == m.key) {
        mine = (uint32_t)s;
        break;
      }
      s = (s + 1) & mask;
    }
    if (mine != MERGE_NONE) {
      atomicAdd(&table[mine].count, 1u);
      atomicMin(&table[mine].first, (uint32_t)g);
    } else {
      atomicOr(flag, 1u);
    }
  }
  slot_of[g] = mine;
}

__global__ __launch_bounds__(COMPACT_THREADS) void k_map_merge_select(
    long long n_rows, const MergeSlot* __restrict__ table, const uint32_t* __restrict__ slot_of,
    const uint32_t* __restrict__ params, unsigned long long* __restrict__ sums, int32_t* __restrict__ tmax,
    uint64_t* __restrict__ ballots, uint32_t* __restrict__ block_counts, uint32_t* __restrict__ block_removed,
    int32_t* __restrict__ counters) {
  const long long g = (long long)blockIdx.x * COMPACT_THREADS + threadIdx.x;
  if (g == 0) {  // the scans that follow in the stream write [0] and [1]
    counters[2] = 0;  // nothing gathered yet
    counters[3] = (int32_t)params[0];
  }
  bool stays = false, goes = false;
  if (g < n_rows) {
    const uint32_t s = slot_of[g];
    stays = true;
    if (s != MERGE_NONE) {
      const MergeSlot slot = table[s];
      stays = slot.first == (uint32_t)g;
      if (stays && slot.count > 1u) {  // the sums of a merged voxel live at its first row
#pragma unroll
        for (int j = 0; j < 6; ++j) sums[6 * (size_t)g + j] = 0ull;
        tmax[g] = INT32_MIN;
      }
    }
    goes = !stays;
  }
  const unsigned long long kept = compact_ballot(stays, ballots);
  const unsigned long long mask[2] = {kept, __ballot(goes)};
  uint32_t sum[2];
  if (compact_block_sums(mask, sum)) {
    block_counts[blockIdx.x] = sum[0];
    block_removed[blockIdx.x] = sum[1];
  }
}

__global__ __launch_bounds__(COMPACT_THREADS) void k_map_merge_sum(
    const float* __restrict__ means, const float* __restrict__ colors, const int32_t* __restrict__ stamps,
    long long n_rows, float inv_h, const MergeSlot* __restrict__ table, const uint32_t* __restrict__ slot_of,
    unsigned long long* sums, int32_t* tmax) {
#pragma clang fp contract(off)
  const long long g = (long long)blockIdx.x * COMPACT_THREADS + threadIdx.x;
  if (g >= n_rows) return;
  const uint32_t s = slot_of[g];
  if (s == MERGE_NONE) return;
  const MergeSlot slot = table[s];
  if (slot.count <= 1u) return;
  const MergeCell m = merge_cell(means, g, inv_h);  // the same arithmetic on the same bits as in the insertion
  unsigned long long* dst = sums + 6 * (size_t)slot.first;  // first < n_rows: a row of this call put it there
#pragma unroll
  for (int a = 0; a < 3; ++a) atomicAdd(dst + a, (unsigned long long)m.q[a]);
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    const float c = fminf(fmaxf(colors[3 * (size_t)g + j], 0.f), 1.f);  // a NaN colour: fmaxf gives the 0
    atomicAdd(dst + 3 + j, (unsigned long long)(uint32_t)rintf(c * 65280.f));
  }
  atomicMax(tmax + slot.first, stamps[g]);
}

__global__ __launch_bounds__(256) void k_map_merge_apply(const int32_t* __restrict__ ids,
                                                        const int32_t* __restrict__ counters, long long n_rows,
                                                        const MergeSlot* __restrict__ table,
                                                        const uint32_t* __restrict__ slot_of,
                                                        const uint32_t* __restrict__ params,
                                                        const unsigned long long* __restrict__ sums,
                                                        const int32_t* __restrict__ tmax, float* __restrict__ out_means,
                                                        float* __restrict__ out_colors, int32_t* __restrict__ out_stamps) {
#pragma clang fp contract(off)
  const long long r = (long long)blockIdx.x * 256 + threadIdx.x;
  long long stored = counters[2];
  stored = stored < n_rows ? stored : n_rows;  // the gather stored no more rows than there are
  if (r >= stored) return;
  const long long id = ids[r];
  if (id < 0 || id >= n_rows) return;  // not an id of this call's gather: nothing is read there
  const uint32_t s = slot_of[id];
  if (s == MERGE_NONE) return;
  const MergeSlot slot = table[s];
  if (slot.count <= 1u || slot.first != (uint32_t)id) return;
  const double k = (double)slot.count, h = (double)__uint_as_float(params[1]);
  const unsigned long long* src = sums + 6 * (size_t)id;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const double c = (double)((int)((slot.key >> (21 * a)) & 0x1fffffull) - MERGE_CELL_BIAS);
    out_means[3 * (size_t)r + a] = (float)((c + (double)src[a] / (65536.0 * k)) * h);
  }
#pragma unroll
  for (int j = 0; j < 3; ++j) out_colors[3 * (size_t)r + j] = (float)((double)src[3 + j] / (65280.0 * k));
  out_stamps[r] = tmax[id];
}

}  // namespace gsl

extern "C" size_t gsl_map_merge_ws_bytes(int64_t n_rows) {
  return gsl::merge_ws_bytes(n_rows < 0x80000000ll ? (long long)n_rows : 0);
}

extern "C" int gsl_map_merge_select(const float* means, const float* colors, const int32_t* stamps, int64_t n_rows,
                                    float inv_h, float h, int32_t* counters, void* ws, size_t ws_bytes, void* stream) {
  if (!means || !colors || !stamps || !counters || !ws) return GSL_ERR_BAD_ARG;
  if (!gsl::map_rows_ok(n_rows)) return GSL_ERR_BAD_ARG;
  if (!(h > 0.f && h < INFINITY) || !(inv_h > 0.f && inv_h < INFINITY)) return GSL_ERR_BAD_ARG;
  if (ws_bytes < gsl_map_merge_ws_bytes(n_rows)) return GSL_ERR_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  const int nb = (int)gsl::compact_blocks(n_rows);
  const gsl::MergeWs w = gsl::merge_ws(ws, (long long)n_rows, nb);
  uint32_t *removed = w.head.extra, *removed_bases = w.head.extra + nb;
  hipLaunchKernelGGL(gsl::k_map_merge_clear, dim3((unsigned)((w.slots + 255) / 256)), dim3(256), 0, st, w.table,
                     w.slots, h, w.params);
  GSL_CHECK_LAUNCH();
  hipLaunchKernelGGL(gsl::k_map_merge_insert, dim3(nb), dim3(gsl::COMPACT_THREADS), 0, st, means, (long long)n_rows,
                     inv_h, w.table, w.slots, w.slot_of, w.params);
  GSL_CHECK_LAUNCH();
  hipLaunchKernelGGL(gsl::k_map_merge_select, dim3(nb), dim3(gsl::COMPACT_THREADS), 0, st, (long long)n_rows, w.table,
                     w.slot_of, w.params, w.sums, w.tmax, w.head.ballots, w.head.counts, removed, counters);
  GSL_CHECK_LAUNCH();
  gsl::launch_count_scan(st, w.head.counts, nb, w.head.bases, counters);
  GSL_CHECK_LAUNCH();
  gsl::launch_count_scan(st, removed, nb, removed_bases, counters + 1);
  GSL_CHECK_LAUNCH();
  hipLaunchKernelGGL(gsl::k_map_merge_sum, dim3(nb), dim3(gsl::COMPACT_THREADS), 0, st, means, colors, stamps,
                     (long long)n_rows, inv_h, w.table, w.slot_of, w.sums, w.tmax);
  GSL_CHECK_LAUNCH();
  return GSL_OK;
}

extern "C" int gsl_map_merge_apply(const int32_t* ids, const int32_t* counters, int64_t n_rows, float* out_means,
                                   float* out_colors, int32_t* out_stamps, void* ws, size_t ws_bytes, void* stream) {
  if (!ids || !counters || !out_means || !out_colors || !out_stamps || !ws) return GSL_ERR_BAD_ARG;
  if (!gsl::map_rows_ok(n_rows)) return GSL_ERR_BAD_ARG;
  if (ws_bytes < gsl_map_merge_ws_bytes(n_rows)) return GSL_ERR_WORKSPACE;
  const int nb = (int)gsl::compact_blocks(n_rows);
  const gsl::MergeWs w = gsl::merge_ws(ws, (long long)n_rows, nb);
  hipLaunchKernelGGL(gsl::k_map_merge_apply, dim3((unsigned)((n_rows + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                     ids, counters, (long long)n_rows, w.table, w.slot_of, w.params, w.sums, w.tmax, out_means,
                     out_colors, out_stamps);
  GSL_CHECK_LAUNCH();
  return GSL_OK;
}
