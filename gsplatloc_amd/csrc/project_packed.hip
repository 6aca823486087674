// Packed projection (gsplat's fully_fused_projection(packed=True)): of the C*N (camera, Gaussian) pairs only those the
// dense kernel gives radii > 0 get an output row, in ascending order of camera * N + gaussian, so everything after
// the cull costs what is visible.  All cameras in one launch; the per-pair arithmetic is project_pair() of
// project_dev.h, the dense kernel's, so a kept row has the dense row's bits.
//
// Order-preserving compaction (compact_dev.h) in two passes over the pairs, one thread per pair:
//   k_packed_project<false>  evaluates the cull and records it; the scan's total -> nnz;
//   k_packed_project<true>   the lanes whose ballot bit is set evaluate the pair again and store at their position.
// The camera is loaded per lane (a wave may straddle two cameras when N % 64 != 0); the 25 floats of one camera are
// one or two cache lines that every lane of the wave hits.  HBM-bound: 40 B read per pair twice, 32 B (+ 16 B of
// ids) written per kept row.
//
// Backward: one thread per packed row, project_vjp<FULL> as in k_project_bwd.  Gaussian gradients go to dense [N,.]
// arrays (plain stores for one camera, where a Gaussian has at most one row; float atomics for several) or to
// [nnz,.] value rows of a sparse gradient (plain stores).  v_viewmats: one partial row per (workgroup, camera it
// touches) at slot workgroup + camera -- rows are sorted by camera, so the slots of touched pairs are distinct -- and
// a fixed-order reduction per camera over the workgroups its rows span.
//
// Row gather (k_gather_rows) and its vjp (k_scatter_rows, k_scatter_add_rows): x[gaussian_ids] / x[camera_ids] for the
// opacities, colours, means and camera positions the packed pipeline reads per row.
#include "compact_dev.h"
#include "gsloc_internal.h"
#include "project_dev.h"

namespace gsl {

template <bool FILL>
__global__ __launch_bounds__(COMPACT_THREADS) void k_packed_project(
    const float* __restrict__ means, const float* __restrict__ quats, const float* __restrict__ scales,
    const float* __restrict__ viewmats, const float* __restrict__ Ks, int C, int N, int W, int H, float eps2d,
    float near_plane, float far_plane, float radius_clip, uint64_t* __restrict__ ballots,
    uint32_t* __restrict__ block_counts, const uint32_t* __restrict__ block_bases, long long capacity,
    int64_t* __restrict__ camera_ids, int64_t* __restrict__ gaussian_ids, int32_t* __restrict__ radii,
    float* __restrict__ means2d, float* __restrict__ depths, float* __restrict__ conics, float* __restrict__ comps) {
  const long long total = (long long)C * N;
  const long long g = (long long)blockIdx.x * COMPACT_THREADS + threadIdx.x;
  bool eval = g < total;
  if (FILL) eval = eval && compact_kept(ballots);
  int cam_id = 0, i = 0;
  ProjOut o;
  o.radius = 0; o.mx = o.my = o.depth = o.ca = o.cb = o.cc = o.comp = 0.f;
  if (eval) {
    cam_id = (int)(g / N);
    i = (int)(g - (long long)cam_id * N);
    Cam cam = load_cam(viewmats + 16 * (size_t)cam_id, Ks + 9 * (size_t)cam_id);
    o = project_pair(means, quats, scales, i, cam, W, H, eps2d, near_plane, far_plane, radius_clip);
  }
  if (!FILL) {
    compact_record(o.radius > 0, ballots, block_counts);
  } else {
    const long long pos = compact_position(ballots, block_bases);
    if (eval && pos < capacity) {
      camera_ids[pos] = cam_id;
      gaussian_ids[pos] = i;
      radii[pos] = o.radius;
      means2d[2 * (size_t)pos] = o.mx;
      means2d[2 * (size_t)pos + 1] = o.my;
      depths[pos] = o.depth;
      conics[3 * (size_t)pos] = o.ca;
      conics[3 * (size_t)pos + 1] = o.cb;
      conics[3 * (size_t)pos + 2] = o.cc;
      if (comps) comps[pos] = o.comp;
    }
  }
}

// Gaussian gradients go to row r of [nnz,.] value arrays (sparse != 0) or to row gaussian_ids[r] of [N,.] arrays; ATOMIC:
// several rows may share a Gaussian (dense outputs, more than one camera).  One camera's dense and sparse gradients come
// from the same instance: only the store address differs.
template <bool FULL, bool ATOMIC>
__global__ __launch_bounds__(256) void k_packed_project_bwd(
    const float* __restrict__ means, const float* __restrict__ quats, const float* __restrict__ scales,
    const float* __restrict__ viewmats, const float* __restrict__ Ks, int C, int N, int W, int H, float eps2d,
    long long nnz, int sparse, const int64_t* __restrict__ camera_ids, const int64_t* __restrict__ gaussian_ids,
    const float* __restrict__ conics, const float* __restrict__ comps, const float* __restrict__ v_means2d,
    const float* __restrict__ v_depths, const float* __restrict__ v_conics, const float* __restrict__ v_comps,
    float* __restrict__ v_means, float* __restrict__ v_quats, float* __restrict__ v_scales,
    float* __restrict__ partials /* [gridDim.x + C - 1][12] or null */) {
  const long long r = (long long)blockIdx.x * 256 + threadIdx.x;
  float vRt[12];  // v_R (9, row-major) then v_t (3)
#pragma unroll
  for (int k = 0; k < 12; ++k) vRt[k] = 0.f;
  int cam_id = -1, i = -1;
  if (r < nnz) {
    cam_id = (int)camera_ids[r];
    i = (int)gaussian_ids[r];
    if (cam_id < 0 || cam_id >= C || i < 0 || i >= N) cam_id = -1;  // ids that are not this call's: no row, no access
  }
  if (cam_id >= 0) {
    Cam cam = load_cam(viewmats + 16 * (size_t)cam_id, Ks + 9 * (size_t)cam_id);
    float vmean[3] = {0.f, 0.f, 0.f}, vq[4] = {0.f, 0.f, 0.f, 0.f}, vs[3] = {0.f, 0.f, 0.f};
    ProjMid p;
    float q[4], s[3];
    load_gaussian(means, quats, scales, i, cam, p, q, s);
    p.covar = quat_scale_to_covar(q, s);
    p.covar_c = mul_bt(mul(cam.R, p.covar), cam.R);
    persp_mid(cam, W, H, p);
    bool has_comp = v_comps != nullptr;
    project_vjp<FULL>(cam, eps2d, p, q, s, conics[3 * (size_t)r], conics[3 * (size_t)r + 1], conics[3 * (size_t)r + 2],
                      v_means2d[2 * (size_t)r], v_means2d[2 * (size_t)r + 1], v_depths[r], v_conics[3 * (size_t)r],
                      v_conics[3 * (size_t)r + 1], v_conics[3 * (size_t)r + 2], has_comp, has_comp ? comps[r] : 0.f,
                      has_comp ? v_comps[r] : 0.f, vRt, vmean, vq, vs);
    if (FULL) {
      const size_t row = sparse ? (size_t)r : (size_t)i;
      if (ATOMIC) {
#pragma unroll
        for (int k = 0; k < 3; ++k) atomicAdd(v_means + 3 * row + k, vmean[k]);
#pragma unroll
        for (int k = 0; k < 4; ++k) atomicAdd(v_quats + 4 * row + k, vq[k]);
#pragma unroll
        for (int k = 0; k < 3; ++k) atomicAdd(v_scales + 3 * row + k, vs[k]);
      } else {
#pragma unroll
        for (int k = 0; k < 3; ++k) v_means[3 * row + k] = vmean[k];
#pragma unroll
        for (int k = 0; k < 4; ++k) v_quats[4 * row + k] = vq[k];
#pragma unroll
        for (int k = 0; k < 3; ++k) v_scales[3 * row + k] = vs[k];
      }
    }
  }
  if (partials != nullptr) {
    // the rows of this workgroup are sorted by camera: one deterministic block reduction (wave butterfly -> LDS -> 12
    // lanes) per camera between its first and its last row's
    __shared__ float red[4][12];
    const long long first = (long long)blockIdx.x * 256;
    const long long last = (first + 255 < nnz ? first + 255 : nnz - 1);
    const int c_lo = max(0, min(C - 1, (int)camera_ids[first])), c_hi = max(0, min(C - 1, (int)camera_ids[last]));
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    for (int cc = c_lo; cc <= c_hi; ++cc) {
#pragma unroll
      for (int k = 0; k < 12; ++k) {
        float sum = wave_sum(cam_id == cc ? vRt[k] : 0.f);
        if (lane == 0) red[wv][k] = sum;
      }
      __syncthreads();
      if (threadIdx.x < 12)
        partials[((size_t)blockIdx.x + cc) * 12 + threadIdx.x] =
            red[0][threadIdx.x] + red[1][threadIdx.x] + red[2][threadIdx.x] + red[3][threadIdx.x];
      __syncthreads();
    }
  }
}

// One workgroup per camera: its rows are [lower_bound(c), lower_bound(c + 1)) of camera_ids; sums the partial rows of
// the workgroups they span in a fixed order -> v_viewmats[c] (row 3 zero; all zero for a camera without rows).
__global__ __launch_bounds__(256) void k_packed_reduce_viewmat(const float* __restrict__ partials,
                                                              const int64_t* __restrict__ camera_ids, long long nnz,
                                                              float* __restrict__ v_viewmats) {
  const int cc = blockIdx.x;
  long long bound[2];
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    long long lo = 0, hi = nnz;
    while (lo < hi) {
      long long mid = (lo + hi) >> 1;
      if (camera_ids[mid] < cc + k) lo = mid + 1;
      else hi = mid;
    }
    bound[k] = lo;
  }
  __shared__ float red[4][12];
  float acc[12];
#pragma unroll
  for (int k = 0; k < 12; ++k) acc[k] = 0.f;
  if (bound[1] > bound[0]) {
    const long long b_lo = bound[0] >> 8, b_hi = (bound[1] - 1) >> 8;
    for (long long b = b_lo + threadIdx.x; b <= b_hi; b += 256)
#pragma unroll
      for (int k = 0; k < 12; ++k) acc[k] += partials[(size_t)(b + cc) * 12 + k];
  }
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < 12; ++k) {
    float s = wave_sum(acc[k]);
    if (lane == 0) red[wv][k] = s;
  }
  __syncthreads();
  if (threadIdx.x < 16) {
    float v = 0.f;
    int r = threadIdx.x >> 2, c = threadIdx.x & 3;
    if (r < 3) {
      int k = (c < 3) ? (r * 3 + c) : (9 + r);
      v = red[0][k] + red[1][k] + red[2][k] + red[3][k];
    }
    v_viewmats[(size_t)cc * 16 + threadIdx.x] = v;
  }
}

// Rows of a per-Gaussian (or per-camera) array for the packed rows: dst[r] = src[ids[r]], D floats per row, one thread
// per element.  An id outside [0, n_src) gives a zero row.
__global__ __launch_bounds__(256) void k_gather_rows(const float* __restrict__ src, long long n_src, int D,
                                                    const int64_t* __restrict__ ids, long long n_elems,
                                                    float* __restrict__ dst) {
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  if (e >= n_elems) return;
  const long long r = e / D;
  const int k = (int)(e - r * D);
  const long long id = ids[r];
  dst[e] = (id >= 0 && id < n_src) ? src[(size_t)id * D + k] : 0.f;
}

// vjp of the gather, no id twice: v_dst[ids[r]] = v_rows[r], one thread per row.
__global__ __launch_bounds__(256) void k_scatter_rows(const float* __restrict__ v_rows, const int64_t* __restrict__ ids,
                                                     long long nnz, int D, long long n_dst,
                                                     float* __restrict__ v_dst) {
  const long long r = (long long)blockIdx.x * 256 + threadIdx.x;
  if (r >= nnz) return;
  const long long id = ids[r];
  if (id < 0 || id >= n_dst) return;
  for (int k = 0; k < D; ++k) v_dst[(size_t)id * D + k] = v_rows[(size_t)r * D + k];
}

// vjp of the gather, repeated ids: v_dst[ids[r]] += v_rows[r] with float atomics.  A wave takes 64 * GSL_SCATTER_ROWS
// consecutive rows, 64 at a time.  The rows are sorted by camera, so with camera_ids as ids (a handful of rows of v_dst
// take every packed row) all lanes hold the same id for long runs: the lanes then sum privately and the wave adds one
// butterfly sum per run instead of one atomic per row to a single address (1 M rows of one camera: 16 k atomics per
// component serialised at one L2 address took 0.60 ms, 1 k take 0.05 ms).  Mixed ids (gaussian_ids of several
// cameras): one atomic per row and component.
#define GSL_SCATTER_ROWS 16
__global__ __launch_bounds__(256) void k_scatter_add_rows(const float* __restrict__ v_rows,
                                                         const int64_t* __restrict__ ids, long long nnz, int D,
                                                         long long n_dst, float* __restrict__ v_dst) {
  const int lane = threadIdx.x & 63;
  const long long wave_base = ((long long)blockIdx.x * 4 + (threadIdx.x >> 6)) * (64 * GSL_SCATTER_ROWS) + lane;
  for (int k = 0; k < D; ++k) {
    float acc = 0.f;
    int cur = -1;  // id of the run the lanes are summing (wave-uniform), -1: none
    for (int j = 0; j < GSL_SCATTER_ROWS; ++j) {
      const long long r = wave_base + (long long)j * 64;
      long long id = r < nnz ? (long long)ids[r] : -1;
      if (id >= n_dst) id = -1;
      const int first = __builtin_amdgcn_readfirstlane((int)id);  // ids < 2^31 (checked on the host)
      const bool uniform = first >= 0 && __ballot((int)id != first) == 0ull;
      const float v = id >= 0 ? v_rows[(size_t)r * D + k] : 0.f;
      if (uniform && first == cur) {
        acc += v;
      } else {
        if (cur >= 0) {
          const float sum = wave_sum(acc);
          if (lane == 0) atomicAdd(v_dst + (size_t)cur * D + k, sum);
        }
        cur = uniform ? first : -1;
        acc = uniform ? v : 0.f;
        if (!uniform && id >= 0) atomicAdd(v_dst + (size_t)id * D + k, v);
      }
    }
    if (cur >= 0) {
      const float sum = wave_sum(acc);
      if (lane == 0) atomicAdd(v_dst + (size_t)cur * D + k, sum);
    }
  }
}

}  // namespace gsl

extern "C" size_t gsl_project_packed_ws_bytes(int C, int N) {
  return gsl::compact_ws_bytes((C > 0 && N > 0) ? (long long)C * N : 0);
}

// Argument checks shared by the count and the fill pass.
static int packed_check(const float* means, const float* quats, const float* scales, const float* viewmats,
                        const float* Ks, int C, int N, int width, int height, const void* ws, size_t ws_bytes) {
  if (C <= 0 || N < 0 || width <= 0 || height <= 0) return GSL_ERR_BAD_ARG;
  if ((long long)C * N > 0x7FFFFFFFll) return GSL_ERR_BAD_ARG;  // pair indices and nnz are 32-bit
  if (N > 0 && (!means || !quats || !scales || !viewmats || !Ks)) return GSL_ERR_BAD_ARG;
  if (N > 0 && (!ws || ws_bytes < gsl_project_packed_ws_bytes(C, N))) return GSL_ERR_WORKSPACE;
  return GSL_OK;
}

extern "C" int gsl_project_packed_count(const float* means, const float* quats, const float* scales,
                                        const float* viewmats, const float* Ks, int C, int N, int width, int height,
                                        float eps2d, float near_plane, float far_plane, float radius_clip,
                                        int32_t* nnz, void* ws, size_t ws_bytes, void* stream) {
  if (!nnz) return GSL_ERR_BAD_ARG;
  int rc = packed_check(means, quats, scales, viewmats, Ks, C, N, width, height, ws, ws_bytes);
  if (rc != GSL_OK) return rc;
  hipStream_t st = (hipStream_t)stream;
  if (N == 0) return gsl::zero_u32(nnz, 1, st);
  const int nb = (int)gsl::compact_blocks((long long)C * N);
  const gsl::CompactWs w = gsl::compact_ws(ws, nb);
  GSL_CLAMP_DEPTH_WINDOW(near_plane, far_plane);
  hipLaunchKernelGGL(gsl::k_packed_project<false>, dim3(nb), dim3(gsl::COMPACT_THREADS), 0, st, means, quats, scales,
                     viewmats, Ks, C, N, width, height, eps2d, near_plane, far_plane, radius_clip, w.ballots, w.counts,
                     (const uint32_t*)nullptr, 0ll, (int64_t*)nullptr, (int64_t*)nullptr, (int32_t*)nullptr,
                     (float*)nullptr, (float*)nullptr, (float*)nullptr, (float*)nullptr);
  GSL_CHECK_LAUNCH();
  gsl::launch_count_scan(st, w.counts, nb, w.bases, nnz);
  GSL_CHECK_LAUNCH();
  return GSL_OK;
}

extern "C" int gsl_project_packed_fill(const float* means, const float* quats, const float* scales,
                                       const float* viewmats, const float* Ks, int C, int N, int width, int height,
                                       float eps2d, float near_plane, float far_plane, float radius_clip,
                                       int64_t capacity, int64_t* camera_ids, int64_t* gaussian_ids, int32_t* radii,
                                       float* means2d, float* depths, float* conics, float* compensations, void* ws,
                                       size_t ws_bytes, void* stream) {
  if (capacity < 0) return GSL_ERR_BAD_ARG;
  int rc = packed_check(means, quats, scales, viewmats, Ks, C, N, width, height, ws, ws_bytes);
  if (rc != GSL_OK) return rc;
  if (N == 0 || capacity == 0) return GSL_OK;
  if (!camera_ids || !gaussian_ids || !radii || !means2d || !depths || !conics) return GSL_ERR_BAD_ARG;
  const int nb = (int)gsl::compact_blocks((long long)C * N);
  const gsl::CompactWs w = gsl::compact_ws(ws, nb);
  GSL_CLAMP_DEPTH_WINDOW(near_plane, far_plane);
  hipLaunchKernelGGL(gsl::k_packed_project<true>, dim3(nb), dim3(gsl::COMPACT_THREADS), 0, (hipStream_t)stream, means,
                     quats, scales, viewmats, Ks, C, N, width, height, eps2d, near_plane, far_plane, radius_clip,
                     w.ballots, w.counts, w.bases, (long long)capacity, camera_ids, gaussian_ids, radii, means2d,
                     depths, conics, compensations);
  GSL_CHECK_LAUNCH();
  return GSL_OK;
}

extern "C" size_t gsl_project_packed_bwd_ws_bytes(int64_t nnz, int C) {
  // one partial row per (workgroup, camera it touches): slot workgroup + camera
  size_t nb = (size_t)(((nnz > 0 ? nnz : 1) + 255) / 256);
  return (nb + (size_t)(C > 0 ? C : 1) - 1) * 12 * sizeof(float);
}

extern "C" int gsl_project_packed_bwd(const float* means, const float* quats, const float* scales,
                                      const float* viewmats, const float* Ks, int C, int N, int width, int height,
                                      float eps2d, int64_t nnz, const int64_t* camera_ids,
                                      const int64_t* gaussian_ids, const float* conics, const float* compensations,
                                      const float* v_means2d, const float* v_depths, const float* v_conics,
                                      const float* v_compensations, int sparse, float* v_means, float* v_quats,
                                      float* v_scales, float* v_viewmats, void* ws, size_t ws_bytes, void* stream) {
  if (C <= 0 || N < 0 || width <= 0 || height <= 0 || nnz < 0 || nnz > (int64_t)C * N) return GSL_ERR_BAD_ARG;
  if ((long long)C * N > 0x7FFFFFFFll) return GSL_ERR_BAD_ARG;
  const bool full = v_means != nullptr;
  if (full != (v_quats != nullptr) || full != (v_scales != nullptr)) return GSL_ERR_BAD_ARG;
  if (v_compensations && !compensations) return GSL_ERR_BAD_ARG;
  if (nnz > 0 && (!means || !quats || !scales || !viewmats || !Ks || !camera_ids || !gaussian_ids || !conics ||
                  !v_means2d || !v_depths || !v_conics))
    return GSL_ERR_BAD_ARG;
  if (nnz > 0 && v_viewmats && (!ws || ws_bytes < gsl_project_packed_bwd_ws_bytes(nnz, C))) return GSL_ERR_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  // dense outputs are OVERWRITTEN: rows without a packed row are zero
  if (full && !sparse && N > 0) {
    if (gsl::zero_u32(v_means, (size_t)N * 3, st) != GSL_OK || gsl::zero_u32(v_quats, (size_t)N * 4, st) != GSL_OK ||
        gsl::zero_u32(v_scales, (size_t)N * 3, st) != GSL_OK)
      return GSL_ERR_HIP;
  }
  if (nnz == 0) {
    if (v_viewmats && gsl::zero_u32(v_viewmats, (size_t)C * 16, st) != GSL_OK) return GSL_ERR_HIP;
    return GSL_OK;
  }
  if (!full && !v_viewmats) return GSL_OK;
  const int grid = (int)((nnz + 255) / 256);
  float* partials = v_viewmats ? (float*)ws : nullptr;
#define GSL_PACKED_BWD(FULL, ATOMIC)                                                                                 \
  hipLaunchKernelGGL((gsl::k_packed_project_bwd<FULL, ATOMIC>), dim3(grid), dim3(256), 0, st, means, quats, scales, \
                     viewmats, Ks, C, N, width, height, eps2d, (long long)nnz, sparse, camera_ids, gaussian_ids,    \
                     conics, compensations, v_means2d, v_depths, v_conics, v_compensations, v_means, v_quats,       \
                     v_scales, partials)
  if (!full) GSL_PACKED_BWD(false, false);
  else if (sparse || C == 1) GSL_PACKED_BWD(true, false);
  else GSL_PACKED_BWD(true, true);
#undef GSL_PACKED_BWD
  GSL_CHECK_LAUNCH();
  if (v_viewmats) {
    hipLaunchKernelGGL(gsl::k_packed_reduce_viewmat, dim3(C), dim3(256), 0, st, (const float*)partials, camera_ids,
                       (long long)nnz, v_viewmats);
    GSL_CHECK_LAUNCH();
  }
  return GSL_OK;
}

extern "C" int gsl_gather_rows(const float* src, int64_t n_src, int D, const int64_t* ids, int64_t nnz, float* dst,
                               void* stream) {
  if (n_src < 0 || D <= 0 || nnz < 0 || nnz > 0x7FFFFFFFll || (long long)nnz * D > ((long long)1 << 38))
    return GSL_ERR_BAD_ARG;
  if (nnz == 0) return GSL_OK;
  if (!ids || !dst || (n_src > 0 && !src)) return GSL_ERR_BAD_ARG;
  const long long n_elems = (long long)nnz * D;
  hipLaunchKernelGGL(gsl::k_gather_rows, dim3((unsigned)((n_elems + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                     src, (long long)n_src, D, ids, n_elems, dst);
  GSL_CHECK_LAUNCH();
  return GSL_OK;
}

extern "C" int gsl_scatter_add_rows(const float* v_rows, const int64_t* ids, int64_t nnz, int D, int64_t n_dst,
                                    int unique, float* v_dst, void* stream) {
  if (n_dst < 0 || n_dst > 0x7FFFFFFFll || D <= 0 || nnz < 0 || nnz > 0x7FFFFFFFll) return GSL_ERR_BAD_ARG;
  if (n_dst == 0) return GSL_OK;
  if (!v_dst || (nnz > 0 && (!v_rows || !ids))) return GSL_ERR_BAD_ARG;
  hipStream_t st = (hipStream_t)stream;
  if (gsl::zero_u32(v_dst, (size_t)n_dst * D, st) != GSL_OK) return GSL_ERR_HIP;  // v_dst is OVERWRITTEN
  if (nnz == 0) return GSL_OK;
  if (unique)
    hipLaunchKernelGGL(gsl::k_scatter_rows, dim3((unsigned)((nnz + 255) / 256)), dim3(256), 0, st, v_rows, ids,
                       (long long)nnz, D, (long long)n_dst, v_dst);
  else
    hipLaunchKernelGGL(gsl::k_scatter_add_rows, dim3((unsigned)((nnz + 256 * GSL_SCATTER_ROWS - 1) /
                                                                (256 * GSL_SCATTER_ROWS))),
                       dim3(256), 0, st, v_rows, ids, (long long)nnz, D, (long long)n_dst, v_dst);
  GSL_CHECK_LAUNCH();
  return GSL_OK;
}
