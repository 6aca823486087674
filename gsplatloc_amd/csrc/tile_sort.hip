// The per-tile sort: every tile's list of (depth bits, Gaussian index) keys -- its span of the packed key array after the
// scatter of two-pass binning (binning.hip, fused_project.hip), or its fixed-capacity bin after a binned projection -- is
// sorted by one wave in registers or by one workgroup in LDS, and leaves as flatten_ids (+ gsplat's isect_ids, + the
// sorted keys).  The composite key makes the result independent of scatter order and identical to a stable global sort
// of the gsplat key.  Lists too long for one workgroup are sorted by several (gsl_long_sort).  The device pieces the
// compositing forward shares when it sorts its own bin are in sort_dev.h.
#include <atomic>
#include <cstdlib>
#include <cstring>
#include "gsloc_internal.h"
#include "long_dev.h"
#include "sort_dev.h"

namespace gsl {

#define GSL_SORT_LDS_CAP 4096  // keys per LDS block of the long-list sort (32 KiB: the wave sorts are limited to four workgroups per CU by their registers anyway)

// Ascending-only bitonic network on n (arbitrary) 64-bit keys; comparators whose upper index
// falls past n are skipped (equivalent to +inf padding).  One comparator sub-step in global memory: used by the
// long-list sort below for the sub-steps that cross 4096-key blocks.
__device__ __forceinline__ void bitonic_flip_step(uint64_t* a, int n, int half, int k, int tid, int nthreads) {
  int hk = k >> 1;
  for (int i = tid; i < half; i += nthreads) {
    int blk = i / hk, off = i - blk * hk;
    int lo = blk * k + off;
    int hi = blk * k + (k - 1 - off);
    if (hi < n) {
      uint64_t x = a[lo], y = a[hi];
      if (x > y) { a[lo] = y; a[hi] = x; }
    }
  }
  __syncthreads();
}
__device__ __forceinline__ void bitonic_half_step(uint64_t* a, int n, int half, int j, int tid, int nthreads) {
  for (int i = tid; i < half; i += nthreads) {
    int blk = i / j, off = i - blk * j;
    int lo = blk * 2 * j + off;
    int hi = lo + j;
    if (hi < n) {
      uint64_t x = a[lo], y = a[hi];
      if (x > y) { a[lo] = y; a[hi] = x; }
    }
  }
  __syncthreads();
}

// LDS version for a 256-thread workgroup.  Each of `nw` working waves owns a contiguous segment
// of S = P/nw keys; every sub-step whose comparator block fits inside a segment needs no
// workgroup barrier (a wave's LDS operations complete in order), which leaves 2-5 s_barriers
// per sort instead of log^2(P)/2.
__device__ __forceinline__ void bitonic_sort_lds(uint64_t* a, int n, int tid) {
  int lgP = 0;
  while ((1 << lgP) < n) ++lgP;
  int P = 1 << lgP;
  if (P < 2) return;
  int nw = P >= 512 ? 4 : (P >= 256 ? 2 : 1);
  int S = P / nw;           // keys per wave segment
  int pairs_w = S >> 1;     // comparators per wave per sub-step
  int wv = tid >> 6, lane = tid & 63;
  bool work = wv < nw;
  int pbase = wv * pairs_w;
  for (int lk = 1; lk <= lgP; ++lk) {  // stage k = 2^lk
    int k = 1 << lk, hk = k >> 1;
    if (work) {
      for (int q = lane; q < pairs_w; q += 64) {
        int i = pbase + q;
        int off = i & (hk - 1);
        int base = (i >> (lk - 1)) << lk;
        int lo = base + off;
        int hi = base + (k - 1 - off);
        if (hi < n) {
          uint64_t x = a[lo], y = a[hi];
          if (x > y) { a[lo] = y; a[hi] = x; }
        }
      }
    }
    if (k > S) __syncthreads();
    else wave_lds_fence();
    for (int lj = lk - 2; lj >= 0; --lj) {  // distance j = 2^lj
      int j = 1 << lj;
      if (work) {
        for (int q = lane; q < pairs_w; q += 64) {
          int i = pbase + q;
          int lo = ((i >> lj) << (lj + 1)) + (i & (j - 1));
          int hi = lo + j;
          if (hi < n) {
            uint64_t x = a[lo], y = a[hi];
            if (x > y) { a[lo] = y; a[hi] = x; }
          }
        }
      }
      // a barrier is needed whenever this or the next sub-step crosses wave segments
      bool cross = (2 * j > S) || (j > 1 ? (j > S) : (2 * k > S));
      if (cross) __syncthreads();
      else wave_lds_fence();
    }
  }
  __syncthreads();
}

// Lists longer than the LDS capacity (a pile of splats in one tile: e.g. the invalid pixels of a TUM depth frame,
// which all sit at the previous camera's origin).  Same network, run block-wise: every stage k <= CAP is the LDS sort
// of one aligned CAP-key block; of a stage k > CAP only the sub-steps at distance >= CAP touch global memory, the
// remaining log2(CAP) sub-steps stay inside aligned blocks and run in LDS.  For n = 24 k: 6 global sub-steps
// instead of 120.
__device__ __forceinline__ void bitonic_sort_long(uint64_t* a, int n, uint64_t* lds, int tid) {
  constexpr int CAP = GSL_SORT_LDS_CAP;
  int nblk = (n + CAP - 1) / CAP;
  for (int b = 0; b < nblk; ++b) {
    int nb = min(CAP, n - b * CAP);
    __syncthreads();
    for (int i = tid; i < nb; i += 256) lds[i] = a[b * CAP + i];
    __syncthreads();
    bitonic_sort_lds(lds, nb, tid);
    for (int i = tid; i < nb; i += 256) a[b * CAP + i] = lds[i];
  }
  __syncthreads();
  int P = CAP;
  while (P < n) P <<= 1;
  int half = P >> 1;
  for (int k = 2 * CAP; k <= P; k <<= 1) {
    bitonic_flip_step(a, n, half, k, tid, 256);
    for (int j = k >> 2; j >= CAP; j >>= 1) bitonic_half_step(a, n, half, j, tid, 256);
    for (int b = 0; b < nblk; ++b) {
      int nb = min(CAP, n - b * CAP);
      for (int i = tid; i < nb; i += 256) lds[i] = a[b * CAP + i];
      __syncthreads();
      for (int j = CAP >> 1; j >= 1; j >>= 1) bitonic_half_step(lds, nb, CAP >> 1, j, tid, 256);
      for (int i = tid; i < nb; i += 256) a[b * CAP + i] = lds[i];
      __syncthreads();
    }
  }
}

// ------------------------------------------------------------------------------------------------
// Per-tile sort, one WAVE per tile: the same ascending bitonic network, with the keys held in registers.
// Element e = lane * KPT + r lives in register r of lane `lane` (KPT = 4 .. 32 keys per lane, P = 64 KPT >= n, padded
// with +inf).  Comparator distances below KPT are register-to-register (no data movement at all: 34 of the 55
// sub-steps at P = 1024), the others exchange through the cross-lane network (ds_bpermute, no memory), and nothing
// needs a barrier or LDS.  Measured against the LDS version it replaces: see DESIGN.md.  Lists longer than 2048
// entries (a pile of splats in one tile) are sorted by the whole workgroup block-wise, bitonic_sort_long.
// ------------------------------------------------------------------------------------------------
// I/O (round 4): the kernel WITHOUT the network took as long as with it -- its 47 us at R were the loads and stores: lane L
// holding elements 16 L .. 16 L + 15 reads (and writes) 64 different cache lines per instruction.  The network does not care
// where an input key starts, so the keys are loaded lane-interleaved (element r * 64 + L: one 512-byte run per instruction);
// the sorted ids are transposed through the wave's own 8 KiB of LDS (rows rotated by the lane: no bank pile-up) and leave as
// contiguous 256-byte runs.  `ids_lds`: 2048 ints private to this wave.
template <int LK>
__device__ __forceinline__ void wave_sort_tile(const uint64_t* __restrict__ src, int n, long long s, int t, int lane,
                                               uint64_t* __restrict__ keys_out, int32_t* __restrict__ flatten_ids,
                                               int64_t* __restrict__ isect_ids, int64_t cam_enc,
                                               const int32_t* __restrict__ storage_of, int32_t* ids_lds,
                                               const RowClear clr, int clr_part) {
  constexpr int KPT = 1 << LK;
  uint64_t k[KPT];
  int e0 = lane * KPT;
#pragma unroll
  for (int r = 0; r < KPT; ++r) k[r] = (r * 64 + lane < n) ? src[r * 64 + lane] : GSL_SORT_PAD;
  keys_arrived();
  if (clr.rows) clr.run(clr_part, lane, 64);  // (this wave's part of the gradient rows: see RowClear)
  wave_sort_regs<LK>(k, lane);
  if (LK <= 4 && !isect_ids && !keys_out) {  // (32 keys per lane: the ids' registers would cost the instance a wave per SIMD)
#pragma unroll
    for (int r = 0; r < KPT; ++r)
      ids_lds[e0 + ((r + lane) & (KPT - 1))] = (e0 + r < n) ? list_id(storage_of, k[r]) : 0;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll
    for (int r = 0; r < KPT; ++r) {
      const int e = r * 64 + lane, row = e >> LK, col = e & (KPT - 1);
      if (e < n) flatten_ids[s + e] = ids_lds[row * KPT + ((col + row) & (KPT - 1))];
    }
    return;
  }
#pragma unroll
  for (int r = 0; r < KPT; ++r)
    if (e0 + r < n) {
      uint64_t v = k[r];
      flatten_ids[s + e0 + r] = list_id(storage_of, v);
      if (isect_ids) isect_ids[s + e0 + r] = cam_enc | ((int64_t)t << 32) | (int64_t)(v >> 32);
      if (keys_out) keys_out[s + e0 + r] = v;
    }
}

#define GSL_SORT_WAVE_MAX 2048  // longest list one wave sorts in registers (32 keys per lane)

// Four tiles per 256-thread workgroup, one per wave; write flatten_ids (+ gsplat-style isect_ids, + the sorted keys
// when the deterministic backward wants them).  The unsorted keys of a tile are its span of `keys`, or its
// fixed-capacity bin (binned projection).
// counts != nullptr (binned projection, launched over ALL tiles): tile_offsets is an OUTPUT -- every workgroup adds up
// the sizes of the tiles before its own (a few coalesced loads per thread) and its waves write the offsets of their
// tiles, the last one also the total; a tile that outgrew its bin keeps bin_cap entries and raises flags[1] (its size
// goes to flags[2]).  The separate single-workgroup scan launch disappears; the counters are cleared later by the
// compositing forward (every workgroup may still be reading them here).
// MAXLK = 4 / 5: the longest list one wave sorts in registers is 1024 / 2048 keys; longer ones go to the workgroup's LDS
// sort below.  The 32-keys-per-lane network is what sets the kernel's register count (141 VGPR once every compare is a
// ballot: three waves per SIMD, one fewer than a frame of 3 225 tiles needs to be resident at once), so frames whose lists
// are expected to stay below 1024 keys run the instance without it (gsl_tile_sort_keys).
// The offsets of the binned mode (binned_tile_span, sort_dev.h, for four tiles at once) and the write-out of a key
// (write_sorted_key) are written out in this kernel and in wave_sort_tile: with the shared functions in their place the
// compiler allocates the registers of the whole kernel differently, and this is the kernel whose schedule was tuned.
// clr (gsl_fused_bin_clear): the launch also zeroes the gradient rows, one part per wave, whatever the wave does with its
// tile -- behind its key loads when it sorts one in registers (RowClear), at once when its tile is empty, past the strip
// or left to the workgroup's long-list sort.
template <int MAXLK>
__global__ __launch_bounds__(256) void k_tile_sort(int32_t* __restrict__ tile_offsets, int tile_begin,
                                                   int n_strip_tiles, long long capacity,
                                                   uint64_t* __restrict__ keys, int32_t* __restrict__ flatten_ids,
                                                   int64_t* __restrict__ isect_ids, int64_t cam_enc,
                                                   int write_sorted_keys, uint64_t* __restrict__ bins, int bin_cap,
                                                   const int32_t* __restrict__ counts, int32_t* __restrict__ n_isects,
                                                   int32_t* __restrict__ flags, int long_min,
                                                   const int32_t* __restrict__ storage_of, const RowClear clr) {
  __shared__ uint64_t skeys[GSL_SORT_LDS_CAP];
  __shared__ int s_scan[8];
  int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  if (counts) {
    int first = tile_begin + blockIdx.x * 4;
    int acc = prefix_count_share(counts, first, bin_cap, tid);
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) acc += __shfl_xor(acc, o, 64);
    int t_own = first + wv;
    int c_own = (blockIdx.x * 4 + wv < n_strip_tiles) ? counts[t_own] : 0;
    if (lane == 0) {
      s_scan[wv] = acc;
      s_scan[4 + wv] = min(c_own, bin_cap);
      if (c_own > bin_cap && flags) { flags[1] = 1; atomicMax(&flags[2], c_own); }
    }
    __syncthreads();
    int base = s_scan[0] + s_scan[1] + s_scan[2] + s_scan[3];
    for (int w = 0; w < wv; ++w) base += s_scan[4 + w];
    if (lane == 0 && blockIdx.x * 4 + wv < n_strip_tiles) {
      tile_offsets[t_own] = base;
      if (blockIdx.x * 4 + wv == n_strip_tiles - 1) {
        tile_offsets[t_own + 1] = base + s_scan[4 + wv];
        if (n_isects) n_isects[0] = base + s_scan[4 + wv];
      }
    }
  }
  // span of tile q of this workgroup in the packed arrays: from the scan above, or from the offsets given
  auto span = [&](int q, long long& s, long long& e) {
    int t = tile_begin + blockIdx.x * 4 + q;
    if (counts) {
      s = s_scan[0] + s_scan[1] + s_scan[2] + s_scan[3];
      for (int w = 0; w < q; ++w) s += s_scan[4 + w];
      e = s + s_scan[4 + q];
    } else {
      s = tile_offsets[t];
      e = tile_offsets[t + 1];
    }
  };
  int local = blockIdx.x * 4 + wv;
  const int clr_part = __builtin_amdgcn_readfirstlane(local);
  bool cleared = false;
  if (local < n_strip_tiles) {
    int t = tile_begin + local;
    long long s, e;
    span(wv, s, e);
    if (e > capacity) e = capacity;
    int n = (int)max(e - s, (long long)0);
    if (bins && n > bin_cap) n = bin_cap;
    const uint64_t* src = bins ? bins + (size_t)t * (size_t)bin_cap : keys + s;
    // sorted keys go to the packed array; in place when that is also the source (every lane has read its keys
    // into registers before any lane writes)
    uint64_t* kout = write_sorted_keys ? keys : nullptr;
    int32_t* const ids_lds = reinterpret_cast<int32_t*>(skeys) + wv * 2048;  // (this wave's quarter of the LDS block)
    if (n > 0 && n <= (64 << MAXLK)) {
      cleared = true;
      if (n <= 256) wave_sort_tile<2>(src, n, s, t, lane, kout, flatten_ids, isect_ids, cam_enc, storage_of, ids_lds, clr, clr_part);
      else if (n <= 512) wave_sort_tile<3>(src, n, s, t, lane, kout, flatten_ids, isect_ids, cam_enc, storage_of, ids_lds, clr, clr_part);
      else if (MAXLK == 4 || n <= 1024) wave_sort_tile<4>(src, n, s, t, lane, kout, flatten_ids, isect_ids, cam_enc, storage_of, ids_lds, clr, clr_part);
      else wave_sort_tile<(MAXLK > 4 ? 5 : 4)>(src, n, s, t, lane, kout, flatten_ids, isect_ids, cam_enc, storage_of, ids_lds, clr, clr_part);
    }
  }
  if (clr.rows && !cleared) clr.run(clr_part, lane, 64);
  // rare: lists too long for one wave, sorted in place by the whole workgroup, one after the other
  for (int q = 0; q < 4; ++q) {
    int lq = blockIdx.x * 4 + q;
    if (lq >= n_strip_tiles) break;
    int t = tile_begin + lq;
    long long s, e;
    span(q, s, e);
    if (e > capacity) e = capacity;
    int n = (int)max(e - s, (long long)0);
    if (bins && n > bin_cap) n = bin_cap;
    if (n <= (64 << MAXLK)) continue;
    if (long_min > 0 && bins && n > long_min) continue;  // sorted by several workgroups: gsl_long_sort
    uint64_t* src = bins ? bins + (size_t)t * (size_t)bin_cap : keys + s;
    __syncthreads();
    bitonic_sort_long(src, n, skeys, tid);
    for (int i = tid; i < n; i += 256) {
      uint64_t k = src[i];
      flatten_ids[s + i] = list_id(storage_of, k);
      if (isect_ids) isect_ids[s + i] = cam_enc | ((int64_t)t << 32) | (int64_t)(k >> 32);
      if (write_sorted_keys && bins) keys[s + i] = k;
    }
  }
}

// ------------------------------------------------------------------------------------------------
// Sort of a LONG tile list by several workgroups (binned mode).  One workgroup sorted such a list block-wise in 1.6 ms
// (23 k keys: the pile of invalid TUM points) -- after the compositing of that list had been split
// over workgroups it was three quarters of the iteration.  Now: every GSL_SORT_SEG-key segment of the list is sorted in
// registers by one wave (k_long_sort_seg, into the packed key array), then `passes` merge passes double the run length,
// one wave per GSL_SORT_SEG outputs (merge path: the two diagonals of the chunk are located by binary search in the two runs,
// the <= GSL_SORT_SEG inputs staged in LDS, every lane merges its share of the outputs), ping-ponging between the packed key array and the
// tile's bin; the last pass writes flatten_ids.  Same result as any stable sort of the (depth bits, id) keys.
// ------------------------------------------------------------------------------------------------
// Head of both kernels: workspace entry g -> its tile, its number as a SORT segment, the tile's span start s and its n keys.
// False: nothing to do for this entry.
__device__ __forceinline__ bool long_sort_entry(const LongWs& w, int g, const int32_t* __restrict__ tile_offsets,
                                                long long capacity, int bin_cap, int& tile, int& sgm, long long& s, int& n) {
  if (g >= w.n_seg[0]) return false;
  tile = w.seg_tile[g];
  sgm = w.seg_idx[g];
  if (tile < 0) return false;  // a tile whose segments did not fit the workspace (flagged by k_long_map)
  // (the map lists compositing segments; the first of every GSL_SORT_SEG / GSL_SEG works as a sort segment)
  if (sgm & (GSL_SORT_SEG / GSL_SEG - 1)) return false;
  sgm >>= GSL_SORT_SEG_LOG2 - GSL_SEG_LOG2;
  s = tile_offsets[tile];
  long long e = tile_offsets[tile + 1];
  if (e > capacity) e = capacity;
  n = (int)min((long long)bin_cap, e - s);
  return true;
}

__global__ __launch_bounds__(64) void k_long_sort_seg(const int32_t* __restrict__ tile_offsets, long long capacity,
                                                      const uint64_t* __restrict__ bins, int bin_cap,
                                                      uint64_t* __restrict__ keys, LongWs w) {
  int tile, sgm, n;
  long long s;
  if (!long_sort_entry(w, blockIdx.x, tile_offsets, capacity, bin_cap, tile, sgm, s, n)) return;
  int lane = threadIdx.x;
  const uint64_t* src = bins + (size_t)tile * (size_t)bin_cap + (size_t)sgm * GSL_SORT_SEG;
  int m = min(GSL_SORT_SEG, n - sgm * GSL_SORT_SEG);
  constexpr int KPL = GSL_SORT_SEG / 64;  // keys per lane
  uint64_t k[KPL];
#pragma unroll
  for (int r = 0; r < KPL; ++r) k[r] = (lane * KPL + r < m) ? src[lane * KPL + r] : GSL_SORT_PAD;
  wave_sort_regs<GSL_SORT_SEG_LOG2 - 6>(k, lane);
  uint64_t* dst = keys + s + (size_t)sgm * GSL_SORT_SEG;
#pragma unroll
  for (int r = 0; r < KPL; ++r)
    if (lane * KPL + r < m) dst[lane * KPL + r] = k[r];
}

// merge_diag by the 64 lanes of a wave together (every lane calls it and gets the result): 64 probes per round instead
// of one, so a diagonal of a 16 k-key run costs 3 dependent global loads instead of 14 (the searches were most of a
// merge pass: 7 us each, eight passes per frame)
__device__ __forceinline__ int merge_diag_wave(const uint64_t* __restrict__ A, int lenA, const uint64_t* __restrict__ B,
                                               int lenB, int d, int lane) {
  int lo = max(0, d - lenB), hi = min(d, lenA);
  while (lo < hi) {  // (wave-uniform)
    int step = (hi - lo + 63) >> 6;
    int mid = lo + lane * step;
    bool pred = mid < hi && A[mid] <= B[d - 1 - mid];  // true exactly for the probes below the answer: a prefix of lanes
    int k = __popcll(__ballot(pred));
    int nhi = (lo + k * step < hi) ? lo + k * step : hi;  // probe k (if there is one) answered "not below"
    lo = k > 0 ? lo + (k - 1) * step + 1 : lo;
    hi = nhi;
  }
  return lo;
}

// pass p: runs of (GSL_SORT_SEG << p) keys -> runs of twice that.  src / dst: the packed key array and the bins, alternating.
__global__ __launch_bounds__(64) void k_long_merge(const int32_t* __restrict__ tile_offsets, long long capacity,
                                                   uint64_t* __restrict__ bins, int bin_cap, uint64_t* __restrict__ keys,
                                                   int pass, int last, int32_t* __restrict__ flatten_ids, LongWs w,
                                                   const int32_t* __restrict__ storage_of) {
  __shared__ uint64_t sk[GSL_SORT_SEG];
  __shared__ int s_split[4];
  int tile, sgm, n;
  long long s;
  if (!long_sort_entry(w, blockIdx.x, tile_offsets, capacity, bin_cap, tile, sgm, s, n)) return;
  int lane = threadIdx.x;
  uint64_t* kbase = keys + s;
  uint64_t* bbase = bins + (size_t)tile * (size_t)bin_cap;
  const uint64_t* src = (pass & 1) ? bbase : kbase;
  uint64_t* dst = (pass & 1) ? kbase : bbase;
  int L = GSL_SORT_SEG << pass;
  int pair_start = (sgm * GSL_SORT_SEG) / (2 * L) * (2 * L);
  int o = sgm * GSL_SORT_SEG - pair_start;
  int lenA = max(0, min(L, n - pair_start)), lenB = max(0, min(L, n - pair_start - L));
  int out_len = min(GSL_SORT_SEG, lenA + lenB - o);
  const uint64_t* A = src + pair_start;
  const uint64_t* B = src + pair_start + L;
  {
    int ia_lo = merge_diag_wave(A, lenA, B, lenB, o, lane);
    int ia_hi = merge_diag_wave(A, lenA, B, lenB, o + out_len, lane);
    if (lane == 0) {
      s_split[0] = ia_lo;
      s_split[1] = o - ia_lo;
      s_split[2] = ia_hi;
      s_split[3] = o + out_len - ia_hi;
    }
  }
  __syncthreads();
  int ia0 = s_split[0], ib0 = s_split[1], na = s_split[2] - ia0, nb = s_split[3] - ib0;
  for (int q = lane; q < na; q += 64) sk[q] = A[ia0 + q];
  for (int q = lane; q < nb; q += 64) sk[na + q] = B[ib0 + q];
  __syncthreads();
  // every lane merges its GSL_SORT_SEG / 64 outputs from the staged pieces
  constexpr int KPL = GSL_SORT_SEG / 64;
  int d0 = min(lane * KPL, out_len), d1 = min(lane * KPL + KPL, out_len);
  int ia = merge_diag(sk, na, sk + na, nb, d0), ib = d0 - ia;
  for (int d = d0; d < d1; ++d) {
    uint64_t v;
    if (ib >= nb || (ia < na && sk[ia] <= sk[na + ib])) v = sk[ia++];
    else v = sk[na + ib++];
    dst[pair_start + o + d] = v;
    if (last) flatten_ids[s + pair_start + o + d] = list_id(storage_of, v);
  }
}

// Same contract as k_tile_sort (offsets from the counters in binned mode, overflow flags, long lists left to
// gsl_long_sort, the gradient rows cleared: one part per workgroup), one tile per workgroup.
__global__ __launch_bounds__(256) void k_tile_sort_wg(int32_t* __restrict__ tile_offsets, int tile_begin,
                                                      int n_strip_tiles, long long capacity,
                                                      uint64_t* __restrict__ keys, int32_t* __restrict__ flatten_ids,
                                                      int64_t* __restrict__ isect_ids, int64_t cam_enc,
                                                      int write_sorted_keys, uint64_t* __restrict__ bins, int bin_cap,
                                                      const int32_t* __restrict__ counts, int32_t* __restrict__ n_isects,
                                                      int32_t* __restrict__ flags, int long_min,
                                                      const int32_t* __restrict__ storage_of, const RowClear clr) {
  __shared__ uint64_t skeys[GSL_SORT_LDS_CAP];
  __shared__ int s_scan[5];
  const int tid = threadIdx.x;
  const int t = tile_begin + blockIdx.x;
  long long s, e;
  if (counts) {
    binned_tile_span(counts, t, (int)blockIdx.x == n_strip_tiles - 1, bin_cap, tile_offsets, n_isects, flags, s_scan, tid, s, e);
  } else {
    s = tile_offsets[t];
    e = tile_offsets[t + 1];
  }
  if (e > capacity) e = capacity;
  int n = (int)max(e - s, (long long)0);
  if (bins && n > bin_cap) n = bin_cap;
  if (clr.rows && (n == 0 || n > 2048)) clr.run(blockIdx.x, tid, 256);  // (no register sort to put the stores behind)
  if (n == 0) return;
  uint64_t* src = bins ? bins + (size_t)t * (size_t)bin_cap : keys + s;
  uint64_t* kout = write_sorted_keys ? keys : nullptr;
  if (n <= 1024) {
    wg_sort_tile<2, true>(src, n, s, t, tid, skeys, kout, flatten_ids, isect_ids, cam_enc, storage_of, clr, blockIdx.x);
  } else if (n <= 2048) {
    wg_sort_tile<3, true>(src, n, s, t, tid, skeys, kout, flatten_ids, isect_ids, cam_enc, storage_of, clr, blockIdx.x);
  } else {
    if (long_min > 0 && bins && n > long_min) return;  // sorted by several workgroups: gsl_long_sort
    bitonic_sort_long(src, n, skeys, tid);
    for (int i = tid; i < n; i += 256)
      write_sorted_key(src[i], s + i, t, write_sorted_keys && bins ? keys : nullptr, flatten_ids, isect_ids, cam_enc, storage_of);
  }
}

}  // namespace gsl

namespace gsl {
// launches of k_tile_sort<4>, k_tile_sort<5>, k_tile_sort_wg issued by this process (host-side diagnostics for the
// tests: which tile-sort kernel a call ran; gsl_dev_tile_sort_launches)
static std::atomic<int64_t> g_tile_sort_launches[3];
}  // namespace gsl

extern "C" int64_t gsl_dev_tile_sort_launches(int variant) {
  if (variant < 0 || variant > 2) return -1;
  return gsl::g_tile_sort_launches[variant].load(std::memory_order_relaxed);
}

extern "C" int gsl_tile_sort(const int32_t* tile_offsets, int tile_begin, int n_strip_tiles, int64_t capacity,
                             uint64_t* sort_keys, int32_t* flatten_ids, int64_t* isect_ids, int64_t cam_enc,
                             void* stream) {
  if (!tile_offsets || tile_begin < 0 || n_strip_tiles < 0 || capacity < 0) return GSL_ERR_BAD_ARG;
  if (n_strip_tiles == 0 || capacity == 0) return GSL_OK;
  if (!sort_keys || !flatten_ids) return GSL_ERR_BAD_ARG;
  return gsl::tile_sort_keys(const_cast<int32_t*>(tile_offsets), tile_begin, n_strip_tiles, capacity, sort_keys, flatten_ids,
                             isect_ids, cam_enc, 0, nullptr, 0, nullptr, nullptr, nullptr, 0, 0, nullptr, nullptr, 0, stream);
}

int gsl::tile_sort_keys(int32_t* tile_offsets, int tile_begin, int n_strip_tiles, int64_t capacity, uint64_t* sort_keys,
                        int32_t* flatten_ids, int64_t* isect_ids, int64_t cam_enc, int write_sorted_keys, uint64_t* bins,
                        int bin_cap, const int32_t* counts, int32_t* n_isects, int32_t* flags, int long_min,
                        int occupied_tiles, const int32_t* storage_of, float* clear_rows, int clear_n, void* stream) {
  if (!tile_offsets || tile_begin < 0 || n_strip_tiles < 0 || capacity < 0) return GSL_ERR_BAD_ARG;
  if (counts && (!bins || tile_begin != 0)) return GSL_ERR_BAD_ARG;  // the scan runs over all tiles, bins only
  if (clear_n < 0 || clear_n > GSL_MAX_GAUSSIANS || (clear_n > 0 && !clear_rows)) return GSL_ERR_BAD_ARG;
  if (clear_n == 0) clear_rows = nullptr;
  if (n_strip_tiles == 0 || (capacity == 0 && !counts))  // no sort launch: the rows are still the caller's to find zero
    return clear_rows ? gsl::zero_u32(clear_rows, (size_t)16 * (size_t)clear_n, (hipStream_t)stream) : GSL_OK;
  if (capacity > 0 && (!sort_keys || !flatten_ids)) return GSL_ERR_BAD_ARG;
  // lists of several hundred keys: one tile per workgroup (waves sort quarters, merged in LDS); short lists: one per wave
  // (occupied_tiles: the tiles that can hold entries -- a strip's, when the launch runs over all tiles of the image)
  const int occ = occupied_tiles > 0 ? occupied_tiles : n_strip_tiles;
  const long long mean_list = capacity / (long long)occ;
  // dev / test switch, read on every call (tests set it per case): "wg" = k_tile_sort_wg, "wave16" / "wave32" =
  // k_tile_sort<4> / <5>, "wave" = the wave kernel with MAXLK by the mean list length; unset or anything else = the
  // library's choice below
  const char* force = getenv("GSL_DEV_TILE_SORT");
  int variant;  // 0 = k_tile_sort<4>, 1 = k_tile_sort<5>, 2 = k_tile_sort_wg
  if (force && !strcmp(force, "wg")) variant = 2;
  else if (force && !strcmp(force, "wave16")) variant = 0;
  else if (force && !strcmp(force, "wave32")) variant = 1;
  // (a latency matter: with more tiles than the chip has room for wave sorts at once, one tile per wave keeps more
  // lists in flight and is as fast or faster -- X: 159 against 169 us; with a strip's few hundred tiles the workgroup
  // kernel's shorter critical path decides)
  else if (!(force && !strcmp(force, "wave")) && mean_list > 320 && occ <= 2048) variant = 2;
  // (capacity carries ~1.3 x head-room: a mean list of <= ~880 keys, whose longest lists stay below 1024 in a frame of
  // evenly spread splats; a tile that does exceed 1024 takes the workgroup's LDS sort -- slower, never wrong)
  else variant = mean_list <= 1150 ? 0 : 1;
  // the gradient rows, 4 float4 each, in one part per workgroup (k_tile_sort_wg) or per wave: a multiple of the part's
  // width, so that every store instruction but a part's last writes one full run
  const int parts = variant == 2 ? n_strip_tiles : (n_strip_tiles + 3) / 4 * 4, width = variant == 2 ? 256 : 64;
  const int n4 = 4 * clear_n;
  const gsl::RowClear clr{(float4*)clear_rows, n4, ((n4 + parts - 1) / parts + width - 1) / width * width};
  auto launch = [&](auto kernel, int tiles_per_wg) {
    hipLaunchKernelGGL(kernel, dim3((n_strip_tiles + tiles_per_wg - 1) / tiles_per_wg), dim3(256), 0, (hipStream_t)stream,
                       tile_offsets, tile_begin, n_strip_tiles, (long long)capacity, sort_keys, flatten_ids, isect_ids,
                       cam_enc, write_sorted_keys, bins, bin_cap, counts, n_isects, flags, long_min, storage_of, clr);
  };
  if (variant == 2) launch(gsl::k_tile_sort_wg, 1);
  else if (variant == 0) launch(gsl::k_tile_sort<4>, 4);
  else launch(gsl::k_tile_sort<5>, 4);
  gsl::g_tile_sort_launches[variant].fetch_add(1, std::memory_order_relaxed);
  GSL_CHECK_LAUNCH();
  return GSL_OK;
}

// Multi-workgroup sort of the long tile lists (binned mode; see k_long_sort_seg).  Call after gsl_fused_bin(long_min).
extern "C" int gsl_long_sort(const int32_t* tile_offsets, int tile_w, int tile_h, int ty0, int ty1, int64_t capacity,
                             uint64_t* bins, int bin_cap, uint64_t* sort_keys, int32_t* flatten_ids, int long_min,
                             void* long_ws, size_t long_ws_bytes, int max_seg, int passes, const int32_t* storage_of,
                             void* stream) {
  if (tile_w <= 0 || tile_h <= 0 || ty0 < 0 || ty1 > tile_h || ty0 > ty1 || capacity < 0 || long_min <= 0 ||
      max_seg <= 0 || passes < 0 || passes > 12 || bin_cap <= 0)
    return GSL_ERR_BAD_ARG;
  if (!tile_offsets || !bins || !sort_keys || !flatten_ids || !long_ws) return GSL_ERR_BAD_ARG;
  if (long_ws_bytes < gsl_long_ws_bytes(max_seg)) return GSL_ERR_WORKSPACE;
  if (ty0 == ty1 || capacity == 0) return GSL_OK;
  hipStream_t st = (hipStream_t)stream;
  gsl::LongWs w = gsl::long_ws_views(long_ws, max_seg);
  gsl::launch_long_map(st, tile_offsets, ty0 * tile_w, (ty1 - ty0) * tile_w, (long long)capacity, long_min, max_seg,
                       GSL_SORT_SEG << passes, w);
  hipLaunchKernelGGL(gsl::k_long_sort_seg, dim3(max_seg), dim3(64), 0, st, tile_offsets, (long long)capacity, bins,
                     bin_cap, sort_keys, w);
  for (int p = 0; p < passes; ++p)
    hipLaunchKernelGGL(gsl::k_long_merge, dim3(max_seg), dim3(64), 0, st, tile_offsets, (long long)capacity, bins, bin_cap,
                       sort_keys, p, p == passes - 1 ? 1 : 0, flatten_ids, w, storage_of);
  GSL_CHECK_LAUNCH();
  return GSL_OK;
}
