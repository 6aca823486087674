// Tile binning for the staged API: which 16x16 screen tiles does each projected Gaussian touch, and in what
// depth order does each tile see them.  Replaces gsplat.isect_tiles (two-pass count/emit +
// a device-wide 64-bit radix sort) and isect_offset_encode (IDX:14360, IDX:14369).
//
// MI355X design: instead of one global radix sort over (tile|depth) keys -- 6 passes x 24 B
// per intersection through HBM -- intersections are bucketed by tile with one counting pass
// (per-tile histogram -> exclusive scan -> scatter: this file) and every tile's list is then sorted on
// (depth bits, Gaussian index) by one wave or workgroup in registers and LDS (tile_sort.hip).  Wave64 lanes that hit
// the same tile are merged with a ballot so hot tiles see one atomic per wave instead of 64.  The scan and the LDS
// scatter also serve the fused pipeline's two-pass path (fused_project.hip).
#include "gsloc_internal.h"
#include "tile_dev.h"

namespace gsl {

// Per-wave merged atomic add of 1 on ctr[key]: lanes holding the same key elect a leader.
// Returns the position (old value + rank among equal lanes) for `active` lanes.
// At most MERGE_ROUNDS leader rounds, the rest fall back to plain atomics (random screen order).
__device__ __forceinline__ int merged_atomic_inc(int32_t* __restrict__ ctr, int key, bool active) {
  int pos = 0;
  unsigned long long todo = __ballot(active);
  int lane = threadIdx.x & 63;
#pragma unroll 1
  for (int round = 0; round < 4 && todo; ++round) {
    int leader = __ffsll((long long)todo) - 1;
    int lkey = __shfl(key, leader, 64);
    unsigned long long same = __ballot(active && key == lkey) & todo;
    int cnt = __popcll(same);
    int base = 0;
    if (lane == leader) base = atomicAdd(&ctr[lkey], cnt);
    base = __shfl(base, leader, 64);
    if ((same >> lane) & 1ull) {
      pos = base + __popcll(same & ((1ull << lane) - 1ull));
      active = false;
    }
    todo &= ~same;
  }
  if (active) pos = atomicAdd(&ctr[key], 1);
  return pos;
}

// Where the scatter kernels find a Gaussian: the staged API's arrays, or the fused pipeline's Q0 records (16-pixel
// tiles; order_ids: the id that goes into the key when the Gaussians are stored in tile order, may be NULL).
struct StagedKeys {
  const float* __restrict__ means2d;
  const int32_t* __restrict__ radii;
  const float* __restrict__ depths;
  int tile_size;
  __device__ __forceinline__ uint64_t locate(int i, float& x, float& y) const {
    x = means2d[2 * (size_t)i];
    y = means2d[2 * (size_t)i + 1];
    return ((uint64_t)__float_as_uint(depths[i]) << 32) | (uint32_t)i;
  }
};
struct RecordKeys {
  const float4* __restrict__ Q0;
  const int32_t* __restrict__ radii;
  const int32_t* __restrict__ order_ids;
  static constexpr int tile_size = 16;
  __device__ __forceinline__ uint64_t locate(int i, float& x, float& y) const {
    float4 q0 = GSL_Q(Q0, i);
    x = q0.x;
    y = q0.y;
    return ((uint64_t)__float_as_uint(q0.z) << 32) | (uint32_t)(order_ids ? order_ids[i] : i);
  }
};
// Strip-clipped tile rectangle of Gaussian i and its (depth bits, id) key; an empty rectangle (and key 0) for i >= N
// and for culled Gaussians.
template <class Src>
__device__ __forceinline__ uint64_t keyed_strip_rect(const Src& src, int i, int N, int tile_w, int tile_h, int ty0,
                                                     int ty1, int& xmin, int& ymin, int& xmax, int& ymax) {
  xmin = ymin = xmax = ymax = 0;
  uint64_t key = 0;
  if (i < N) {
    int r = src.radii[i];
    if (r > 0) {
      float x, y;
      key = src.locate(i, x, y);
      strip_rect(x, y, r, src.tile_size, tile_w, tile_h, ty0, ty1, xmin, ymin, xmax, ymax);
    }
  }
  return key;
}
// The rectangle alone, for the counting kernels.
__device__ __forceinline__ void gauss_strip_rect(const float* __restrict__ means2d, const int32_t* __restrict__ radii,
                                                 int i, int N, int tile_size, int tile_w, int tile_h, int ty0, int ty1,
                                                 int& xmin, int& ymin, int& xmax, int& ymax) {
  xmin = ymin = xmax = ymax = 0;
  if (i < N) {
    int r = radii[i];
    if (r > 0)
      strip_rect(means2d[2 * (size_t)i], means2d[2 * (size_t)i + 1], r, tile_size, tile_w, tile_h, ty0, ty1, xmin, ymin,
                 xmax, ymax);
  }
}

// Walk of a thread's rectangle in which all lanes of the wave iterate together, so that merged_atomic_inc sees them:
// per_tile(tile, active) is called by every lane for as many steps as the wave's largest rectangle has tiles.
template <class F>
__device__ __forceinline__ void wave_walk_rect(int xmin, int ymin, int xmax, int ymax, int tile_w, F per_tile) {
  int w = xmax - xmin, n = w * (ymax - ymin);
  int nmax = n;
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) nmax = max(nmax, __shfl_xor(nmax, o, 64));
  for (int k = 0; k < nmax; ++k) {
    bool act = k < n;
    int t = 0;
    if (act) t = (ymin + k / w) * tile_w + xmin + k % w;
    per_tile(t, act);
  }
}

// ---- strips of more than GSL_MAX_STRIP_TILES tiles: global atomics, merged per wave ---------------------------------
// Pass 1: per-Gaussian tile count (strip-clipped) + per-tile histogram.
__global__ __launch_bounds__(256) void k_isect_count(const float* __restrict__ means2d,
                                                     const int32_t* __restrict__ radii, int N, int tile_size,
                                                     int tile_w, int tile_h, int ty0, int ty1,
                                                     int32_t* __restrict__ tiles_per_gauss,
                                                     int32_t* __restrict__ tile_counts) {
  int i = blockIdx.x * 256 + threadIdx.x;
  int xmin, ymin, xmax, ymax;
  gauss_strip_rect(means2d, radii, i, N, tile_size, tile_w, tile_h, ty0, ty1, xmin, ymin, xmax, ymax);
  if (i < N && tiles_per_gauss) tiles_per_gauss[i] = (xmax - xmin) * (ymax - ymin);
  wave_walk_rect(xmin, ymin, xmax, ymax, tile_w, [&](int t, bool act) { merged_atomic_inc(tile_counts, t, act); });
}

// Pass 2: scatter (depth bits, Gaussian id) into the tile buckets.
__global__ __launch_bounds__(256) void k_isect_scatter(StagedKeys src, int N, int tile_w, int tile_h, int ty0, int ty1,
                                                       const int32_t* __restrict__ tile_offsets,
                                                       int32_t* __restrict__ cursors, long long capacity,
                                                       uint64_t* __restrict__ keys) {
  int i = blockIdx.x * 256 + threadIdx.x;
  int xmin, ymin, xmax, ymax;
  uint64_t key = keyed_strip_rect(src, i, N, tile_w, tile_h, ty0, ty1, xmin, ymin, xmax, ymax);
  wave_walk_rect(xmin, ymin, xmax, ymax, tile_w, [&](int t, bool act) {
    int p = merged_atomic_inc(cursors, t, act);
    if (act) {
      long long pos = (long long)tile_offsets[t] + p;
      if (pos < capacity) keys[pos] = key;
    }
  });
}

// ---- LDS-privatised variants (strip of <= GSL_MAX_STRIP_TILES tiles) -------------------------------------------------
// Each 512-thread workgroup histograms its Gaussians' tiles in LDS (ds_add, no return) and
// touches global memory once per distinct tile: for raster-ordered splats (one per pixel of the
// previous depth frame) that is a few dozen atomics per workgroup instead of one per intersection.
__global__ __launch_bounds__(GSL_BIN_THREADS) void k_isect_count_lds(
    const float* __restrict__ means2d, const int32_t* __restrict__ radii, int N, int tile_size, int tile_w, int tile_h,
    int ty0, int ty1, int32_t* __restrict__ tiles_per_gauss, int32_t* __restrict__ tile_counts) {
  extern __shared__ int s_hist[];
  int nst = (ty1 - ty0) * tile_w, tbase = ty0 * tile_w;
  for (int k = threadIdx.x; k < nst; k += GSL_BIN_THREADS) s_hist[k] = 0;
  __syncthreads();
  int i = blockIdx.x * GSL_BIN_THREADS + threadIdx.x;
  int xmin, ymin, xmax, ymax;
  gauss_strip_rect(means2d, radii, i, N, tile_size, tile_w, tile_h, ty0, ty1, xmin, ymin, xmax, ymax);
  if (i < N && tiles_per_gauss) tiles_per_gauss[i] = (xmax - xmin) * (ymax - ymin);
  for (int y = ymin; y < ymax; ++y)
    for (int x = xmin; x < xmax; ++x) atomicAdd(&s_hist[y * tile_w + x - tbase], 1);
  __syncthreads();
  for (int k = threadIdx.x; k < nst; k += GSL_BIN_THREADS) {
    int c = s_hist[k];
    if (c) atomicAdd(&tile_counts[tbase + k], c);
  }
}

// Scatter of the (depth bits | Gaussian id) keys into the tile buckets: count per tile in LDS, reserve this workgroup's
// span of every bucket it touches, rank inside the span from LDS.
template <class Src>
__global__ __launch_bounds__(GSL_BIN_THREADS) void k_isect_scatter_lds(Src src, int N, int tile_w, int tile_h, int ty0,
                                                                       int ty1, const int32_t* __restrict__ tile_offsets,
                                                                       int32_t* __restrict__ cursors, long long capacity,
                                                                       uint64_t* __restrict__ keys) {
  extern __shared__ int s_mem[];
  int nst = (ty1 - ty0) * tile_w, tbase = ty0 * tile_w;
  int* s_cnt = s_mem;
  int* s_base = s_mem + nst;
  for (int k = threadIdx.x; k < nst; k += GSL_BIN_THREADS) s_cnt[k] = 0;
  __syncthreads();
  int i = blockIdx.x * GSL_BIN_THREADS + threadIdx.x;
  int xmin, ymin, xmax, ymax;
  uint64_t key = keyed_strip_rect(src, i, N, tile_w, tile_h, ty0, ty1, xmin, ymin, xmax, ymax);
  for (int y = ymin; y < ymax; ++y)
    for (int x = xmin; x < xmax; ++x) atomicAdd(&s_cnt[y * tile_w + x - tbase], 1);
  __syncthreads();
  // one returning global atomic per distinct tile reserves this workgroup's span of the bucket;
  // all of a thread's atomics are issued before the first result is consumed
  {
    int res[GSL_MAX_STRIP_TILES / GSL_BIN_THREADS];
#pragma unroll
    for (int u = 0; u < GSL_MAX_STRIP_TILES / GSL_BIN_THREADS; ++u) {
      int k = threadIdx.x + u * GSL_BIN_THREADS;
      int c = (k < nst) ? s_cnt[k] : 0;
      res[u] = c ? atomicAdd(&cursors[tbase + k], c) : 0;
    }
#pragma unroll
    for (int u = 0; u < GSL_MAX_STRIP_TILES / GSL_BIN_THREADS; ++u) {
      int k = threadIdx.x + u * GSL_BIN_THREADS;
      if (k < nst) {
        if (s_cnt[k]) s_base[k] = tile_offsets[tbase + k] + res[u];
        s_cnt[k] = 0;
      }
    }
  }
  __syncthreads();
  for (int y = ymin; y < ymax; ++y)
    for (int x = xmin; x < xmax; ++x) {
      int lt = y * tile_w + x - tbase;
      long long pos = (long long)s_base[lt] + atomicAdd(&s_cnt[lt], 1);
      if (pos < capacity) keys[pos] = key;
    }
}

// Exclusive scan of tile counts (single workgroup) -> offsets[n+1], total, zeroed cursors.  The counts are cleared
// after they are read (the next pass accumulates into them again).
__global__ __launch_bounds__(1024) void k_ftile_scan(int32_t* __restrict__ counts, int n,
                                                     int32_t* __restrict__ offsets, int32_t* __restrict__ n_isects,
                                                     int32_t* __restrict__ cursors) {
  __shared__ int wsum[16];
  __shared__ int carry_s;
  int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  if (tid == 0) carry_s = 0;
  __syncthreads();
  for (int base = 0; base < n; base += 1024) {
    int i = base + tid;
    int v = (i < n) ? counts[i] : 0;
    if (i < n) counts[i] = 0;
    int x = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      int y = __shfl_up(x, o, 64);
      if (lane >= o) x += y;
    }
    if (lane == 63) wsum[wv] = x;
    __syncthreads();
    int woff = 0;
    for (int k = 0; k < wv; ++k) woff += wsum[k];
    int carry = carry_s;
    if (i < n) {
      offsets[i] = carry + woff + x - v;
      cursors[i] = 0;
    }
    __syncthreads();
    if (tid == 1023) carry_s = carry + woff + x;
    __syncthreads();
  }
  if (tid == 0) {
    offsets[n] = carry_s;
    n_isects[0] = carry_s;
  }
}

// isect_tiles(sort=False): emit in Gaussian order at cum_tiles positions.
__global__ __launch_bounds__(256) void k_isect_emit(const float* __restrict__ means2d,
                                                    const int32_t* __restrict__ radii,
                                                    const float* __restrict__ depths,
                                                    const int64_t* __restrict__ cum_tiles, int N, int tile_size,
                                                    int tile_w, int tile_h, int64_t cam_enc, int id_offset,
                                                    int64_t* __restrict__ isect_ids,
                                                    int32_t* __restrict__ flatten_ids) {
  int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= N) return;
  int r = radii[i];
  if (r <= 0) return;
  int xmin, ymin, xmax, ymax;
  tile_rect(means2d[2 * (size_t)i], means2d[2 * (size_t)i + 1], r, tile_size, tile_w, tile_h, xmin, ymin, xmax, ymax);
  int64_t cur = (i == 0) ? 0 : cum_tiles[i - 1];
  int64_t dbits = (int64_t)__float_as_uint(depths[i]);
  for (int y = ymin; y < ymax; ++y)
    for (int x = xmin; x < xmax; ++x) {
      int64_t tile = (int64_t)y * tile_w + x;
      isect_ids[cur] = cam_enc | (tile << 32) | dbits;
      flatten_ids[cur] = id_offset + i;
      ++cur;
    }
}

// isect_offset_encode: offsets[q] = first index whose (cam,tile) >= q.
__global__ __launch_bounds__(256) void k_isect_offsets(const int64_t* __restrict__ isect_ids, long long n,
                                                       int n_cameras, int n_tiles, int tile_n_bits,
                                                       int32_t* __restrict__ offsets) {
  long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  long long total = (long long)n_cameras * n_tiles;
  if (n == 0) {
    if (idx < total) offsets[idx] = 0;
    return;
  }
  if (idx >= n) return;
  int64_t mask = ((int64_t)1 << tile_n_bits) - 1;
  int64_t id = isect_ids[idx];
  long long cur = (id >> (32 + tile_n_bits)) * n_tiles + ((id >> 32) & mask);
  if (idx == 0) {
    for (long long q = 0; q <= cur; ++q) offsets[q] = 0;
  }
  if (idx == n - 1) {
    for (long long q = cur + 1; q < total; ++q) offsets[q] = (int32_t)n;
  }
  if (idx > 0) {
    int64_t pid = isect_ids[idx - 1];
    long long prev = (pid >> (32 + tile_n_bits)) * n_tiles + ((pid >> 32) & mask);
    for (long long q = prev + 1; q <= cur; ++q) offsets[q] = (int32_t)idx;
  }
}

void launch_tile_scan(hipStream_t st, int32_t* counts, int n_tiles, int32_t* tile_offsets, int32_t* n_isects,
                      int32_t* cursors) {
  hipLaunchKernelGGL(k_ftile_scan, dim3(1), dim3(1024), 0, st, counts, n_tiles, tile_offsets, n_isects, cursors);
}

template <class Src>
static void launch_scatter_lds(hipStream_t st, Src src, int N, int tile_w, int tile_h, int ty0, int ty1,
                               const int32_t* tile_offsets, int32_t* cursors, long long capacity, uint64_t* keys) {
  hipLaunchKernelGGL(k_isect_scatter_lds<Src>, dim3((N + GSL_BIN_THREADS - 1) / GSL_BIN_THREADS), dim3(GSL_BIN_THREADS),
                     (size_t)2 * (ty1 - ty0) * tile_w * sizeof(int), st, src, N, tile_w, tile_h, ty0, ty1, tile_offsets,
                     cursors, capacity, keys);
}
void launch_record_scatter(hipStream_t st, const float* Q0, const int32_t* radii, const int32_t* order_ids, int N,
                           int tile_w, int tile_h, int ty0, int ty1, const int32_t* tile_offsets, int32_t* cursors,
                           long long capacity, uint64_t* keys) {
  launch_scatter_lds(st, RecordKeys{(const float4*)Q0, radii, order_ids}, N, tile_w, tile_h, ty0, ty1, tile_offsets,
                     cursors, capacity, keys);
}

}  // namespace gsl

extern "C" size_t gsl_isect_ws_bytes(int n_tiles) {
  // [tile_counts n_tiles][cursors n_tiles]
  return (size_t)2 * (size_t)(n_tiles > 0 ? n_tiles : 1) * sizeof(int32_t);
}

extern "C" int gsl_isect_count(const float* means2d, const int32_t* radii, int N, int tile_size, int tile_w,
                               int tile_h, int ty0, int ty1, int32_t* tiles_per_gauss, int32_t* tile_offsets,
                               int32_t* n_isects, void* ws, size_t ws_bytes, void* stream) {
  if (N < 0 || tile_size <= 0 || tile_w <= 0 || tile_h <= 0 || ty0 < 0 || ty1 > tile_h || ty0 > ty1)
    return GSL_ERR_BAD_ARG;
  if (!tile_offsets || !n_isects || (N > 0 && (!means2d || !radii))) return GSL_ERR_BAD_ARG;
  int n_tiles = tile_w * tile_h;
  if (!ws || ws_bytes < gsl_isect_ws_bytes(n_tiles)) return GSL_ERR_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  int32_t* counts = (int32_t*)ws;
  int32_t* cursors = counts + n_tiles;
  if (gsl::zero_u32(counts, (size_t)n_tiles, st) != GSL_OK) return GSL_ERR_HIP;
  if (N > 0) {
    int nst = (ty1 - ty0) * tile_w;
    if (nst > 0 && nst <= GSL_MAX_STRIP_TILES) {
      hipLaunchKernelGGL(gsl::k_isect_count_lds, dim3((N + GSL_BIN_THREADS - 1) / GSL_BIN_THREADS),
                         dim3(GSL_BIN_THREADS), (size_t)nst * sizeof(int), st, means2d, radii, N, tile_size, tile_w,
                         tile_h, ty0, ty1, tiles_per_gauss, counts);
    } else {
      hipLaunchKernelGGL(gsl::k_isect_count, dim3((N + 255) / 256), dim3(256), 0, st, means2d, radii, N, tile_size,
                         tile_w, tile_h, ty0, ty1, tiles_per_gauss, counts);
    }
    GSL_CHECK_LAUNCH();
  }
  gsl::launch_tile_scan(st, counts, n_tiles, tile_offsets, n_isects, cursors);
  GSL_CHECK_LAUNCH();
  return GSL_OK;
}

extern "C" int gsl_isect_fill(const float* means2d, const int32_t* radii, const float* depths, int N, int tile_size,
                              int tile_w, int tile_h, int ty0, int ty1, int cam_id, int tile_n_bits,
                              const int32_t* tile_offsets, int64_t capacity, uint64_t* sort_keys,
                              int32_t* flatten_ids, int64_t* isect_ids, void* ws, size_t ws_bytes, void* stream) {
  if (N < 0 || tile_size <= 0 || tile_w <= 0 || tile_h <= 0 || ty0 < 0 || ty1 > tile_h || ty0 > ty1 || capacity < 0)
    return GSL_ERR_BAD_ARG;
  if (!tile_offsets) return GSL_ERR_BAD_ARG;
  if (N == 0 || capacity == 0 || ty0 == ty1) return GSL_OK;
  if (!means2d || !radii || !depths || !sort_keys || !flatten_ids) return GSL_ERR_BAD_ARG;
  int n_tiles = tile_w * tile_h;
  if (!ws || ws_bytes < gsl_isect_ws_bytes(n_tiles)) return GSL_ERR_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  int32_t* cursors = (int32_t*)ws + n_tiles;
  int nst = (ty1 - ty0) * tile_w;
  const gsl::StagedKeys src{means2d, radii, depths, tile_size};
  if (nst <= GSL_MAX_STRIP_TILES) {
    gsl::launch_scatter_lds(st, src, N, tile_w, tile_h, ty0, ty1, tile_offsets, cursors, (long long)capacity, sort_keys);
  } else {
    hipLaunchKernelGGL(gsl::k_isect_scatter, dim3((N + 255) / 256), dim3(256), 0, st, src, N, tile_w, tile_h, ty0, ty1,
                       tile_offsets, cursors, (long long)capacity, sort_keys);
  }
  GSL_CHECK_LAUNCH();
  int64_t cam_enc = (int64_t)cam_id << (32 + tile_n_bits);
  return gsl_tile_sort(tile_offsets, ty0 * tile_w, (ty1 - ty0) * tile_w, capacity, sort_keys, flatten_ids, isect_ids,
                       cam_enc, stream);
}

extern "C" int gsl_isect_emit(const float* means2d, const int32_t* radii, const float* depths,
                              const int64_t* cum_tiles, int N, int tile_size, int tile_w, int tile_h, int cam_id,
                              int tile_n_bits, int id_offset, int64_t* isect_ids, int32_t* flatten_ids,
                              void* stream) {
  if (N < 0 || tile_size <= 0 || tile_w <= 0 || tile_h <= 0) return GSL_ERR_BAD_ARG;
  if (N == 0) return GSL_OK;
  if (!means2d || !radii || !depths || !cum_tiles || !isect_ids || !flatten_ids) return GSL_ERR_BAD_ARG;
  int64_t cam_enc = (int64_t)cam_id << (32 + tile_n_bits);
  hipLaunchKernelGGL(gsl::k_isect_emit, dim3((N + 255) / 256), dim3(256), 0, (hipStream_t)stream, means2d, radii,
                     depths, cum_tiles, N, tile_size, tile_w, tile_h, cam_enc, id_offset, isect_ids, flatten_ids);
  GSL_CHECK_LAUNCH();
  return GSL_OK;
}

extern "C" int gsl_isect_offsets(const int64_t* isect_ids, int64_t n_isects, int n_cameras, int n_tiles,
                                 int tile_n_bits, int32_t* offsets, void* stream) {
  if (n_isects < 0 || n_cameras <= 0 || n_tiles <= 0 || !offsets) return GSL_ERR_BAD_ARG;
  if (n_isects > 0 && !isect_ids) return GSL_ERR_BAD_ARG;
  long long work = n_isects > 0 ? (long long)n_isects : (long long)n_cameras * n_tiles;
  hipLaunchKernelGGL(gsl::k_isect_offsets, dim3((unsigned)((work + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                     isect_ids, (long long)n_isects, n_cameras, n_tiles, tile_n_bits, offsets);
  GSL_CHECK_LAUNCH();
  return GSL_OK;
}
