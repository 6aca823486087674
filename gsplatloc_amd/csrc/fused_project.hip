// Fused single-camera render pipeline for GsplatLoc's pose-tracking loop (the hot path):
//   forward : project + SH colour + pack + tile histogram                                                (this file)
//             -> scan -> scatter (binning.hip) -> per-tile sort (tile_sort.hip)
//             -> composite (expected-depth normalisation fused)                                          (raster_px.hip)
//   backward: composite vjp (packed 64-byte gradient rows)            (raster_g16.hip; deterministic: raster_det.hip)
//             -> projection/SH vjp + pose reduction                                                      (fused_project_bwd.hip)
// Same arithmetic as the stage operators (project.hip / binning.hip / raster.hip / sh.hip), which
// restate gsplat.rasterization (IDX:14954) as called from /root/reference/src/my_gsplat/model.py:195-213;
// the difference is data layout and launch count.  This file: the forward projection with its binning (gsl_fused_project,
// gsl_fused_bin) and the exported view of the pipeline's workspace layout (gsloc_internal.h has the layout itself).
//
// HBM layout (SoA of 16-byte records, one per Gaussian, written once by the projection kernel and
// gathered by the compositing kernels with one or two dwordx4 loads):
//   Q0 = (x, y, depth, opacity_eff)   Q1 = (conic_a, conic_b, conic_c, r_cull)   Q2 = (r, g, b, 0)
// r_cull is a conservative radius of the alpha >= 1/255 region, used by the per-quadrant ballot test.
// gsplat's meta tensors (means2d, depths, conics, opacities) are strided views of Q0/Q1 on the host.
#include "gsloc_internal.h"
#include "project_dev.h"
#include "sh_dev.h"
#include "tile_dev.h"

namespace gsl {

// Radius of the smallest disc around the centre that holds the whole alpha >= 1/255 ellipse {sigma <= tau}:
// sqrt(2 tau / lambda_min(conic)).  (Round 2 stored the half-extent of the ellipse's axis-aligned bounding box, which is
// smaller for a rotated anisotropic splat; every user treats the value as conservative -- the forward's pixel boxes,
// the quadrant tests, the 4x4 slabs of the tiny backward -- and the 16-lane-group backward tests the DISC against its
// 4x4 pixel blocks.  Identical for isotropic splats, GsplatLoc's only kind.)
__device__ __forceinline__ float cull_radius(float ca, float cb, float cc, float op) {
  float tau = __logf(255.f * op) * 1.01f + 0.01f;
  float det = ca * cc - cb * cb;
  if (!(tau > 0.f)) return -1.f;  // opacity < 1/255: can never reach the alpha threshold
  if (!(det > 0.f) || !(ca > 0.f) || !(cc > 0.f)) return 1e30f;  // degenerate conic: never cull
  float hd = 0.5f * (ca - cc);
  float root = sqrtf(hd * hd + cb * cb);
  float lmin = det / (0.5f * (ca + cc) + root);  // = mean - root, without the cancellation
  if (!(lmin > 0.f)) return 1e30f;
  return sqrtf(2.f * tau / lmin) * 1.0001f + 1e-3f;
}

// ------------------------------------------------------------------------------------------------
// Forward 1: projection + colour + pack + tile histogram.
// ------------------------------------------------------------------------------------------------
// BINNED: the kernel also reserves each intersection's slot in its tile's fixed-capacity bin (one returning atomic per
// distinct tile per workgroup, ranks inside the workgroup from LDS) and writes the (depth bits | id) key there: the
// separate scatter pass and its second read of the records disappear.  tile_counts ends up holding the tile sizes.
template <bool RGB, bool BINNED>
__global__ __launch_bounds__(GSL_BIN_THREADS) void k_fproject(
    const float* __restrict__ means, const float* __restrict__ quats, const float* __restrict__ scales,
    const float* __restrict__ opacities, const float* __restrict__ colors, int sh_degree, int K_sh,
    const float* __restrict__ V, const float* __restrict__ Kmat, int N, int W, int H, float eps2d, float near_plane,
    float far_plane, float radius_clip, int antialiased, int tile_w, int tile_h, int ty0, int ty1,
    int32_t* __restrict__ radii, float4* __restrict__ Q0, float4* __restrict__ Q1, float4* __restrict__ Q2,
    float* __restrict__ comps, int32_t* __restrict__ tiles_per_gauss, int32_t* __restrict__ tile_counts,
    uint4* __restrict__ Qh, uint64_t* __restrict__ bins, int bin_cap, int32_t* __restrict__ bin_state,
    int32_t* __restrict__ flags, const int32_t* __restrict__ order_ids) {
  extern __shared__ int s_hist[];
  int nst = (ty1 - ty0) * tile_w, tbase = ty0 * tile_w;
  // Counter contract of the binned mode: the tile counters must be zero on entry -- the compositing forward of the
  // previous iteration clears them and marks the state word clean.  A projection that finds the state dirty (a forward
  // was skipped or failed between two projections) raises flags[3] instead of binning on top of stale sizes silently.
  if (BINNED && bin_state && nst > 0 && blockIdx.x == 0 && threadIdx.x == 0) {
    if (atomicExch(bin_state, 1) != 0 && flags) flags[3] = 1;
  }
  // s_hist[nst], s_hist[nst + 1]: lowest / highest strip-tile index a Gaussian of this workgroup touches.  The passes over
  // the counters below cover that range only: with the Gaussians stored in tile order (context.py:_choose_placement) a
  // workgroup's 512 touch a band of two or three tile rows, not the frame's 3 225 tiles (the fixed 16-step loops were a
  // quarter of the kernel's VALU instructions).
  int* const s_rng = s_hist + nst;
  for (int k = threadIdx.x; k < nst; k += GSL_BIN_THREADS) s_hist[k] = 0;
  if (threadIdx.x == 0) { s_rng[0] = nst; s_rng[1] = -1; }
  __syncthreads();
  int i = blockIdx.x * GSL_BIN_THREADS + threadIdx.x;
  Cam cam = load_cam(V, Kmat);
  int xmin = 0, ymin = 0, xmax = 0, ymax = 0;
  uint64_t key = 0;
  if (i < N) {
    ProjMid p;
    float q[4], s[3];
    load_gaussian(means, quats, scales, i, cam, p, q, s);
    // EVERY global load of the thread is issued here, before the first value is used.  Left alone, the compiler sinks each
    // load into the branch that needs it -- mean, then (depth test) rotation and scale, then (visibility test) opacity,
    // then one coefficient triple per turn of the colour loop -- and a wave pays five to seven DEPENDENT memory round
    // trips for 92 bytes (round 4: a wave of this kernel lived 36 k cycles for 3.6 k cycles of arithmetic).  The empty
    // asm consumes all of them at once: one wait.
    float op_in = opacities[i];
    float shc[12];  // the colour itself (sh_degree < 0) or the first four coefficient triples (everything up to degree 1)
#pragma unroll
    for (int k = 0; k < 12; ++k) shc[k] = 0.f;
    if (RGB) {
      if (sh_degree < 0) {
#pragma unroll
        for (int k = 0; k < 3; ++k) shc[k] = colors[3 * (size_t)i + k];
      } else {
        const float* cf = colors + (size_t)i * K_sh * 3;
#pragma unroll
        for (int k = 0; k < 3; ++k) shc[k] = cf[k];
        if (sh_degree >= 1) {  // (one uniform branch for the three triples of degree 1: their loads leave together)
#pragma unroll
          for (int k = 3; k < 12; ++k) shc[k] = cf[k];
        }
      }
    }
    asm volatile("" : "+v"(p.mean[0]), "+v"(p.mean[1]), "+v"(p.mean[2]), "+v"(q[0]), "+v"(q[1]), "+v"(q[2]), "+v"(q[3]),
                 "+v"(s[0]), "+v"(s[1]), "+v"(s[2]), "+v"(op_in), "+v"(shc[0]), "+v"(shc[1]), "+v"(shc[2]), "+v"(shc[3]),
                 "+v"(shc[4]), "+v"(shc[5]), "+v"(shc[6]), "+v"(shc[7]), "+v"(shc[8]), "+v"(shc[9]), "+v"(shc[10]),
                 "+v"(shc[11]));
    int radius = 0;
    float4 o0 = make_float4(0.f, 0.f, 0.f, 0.f), o1 = make_float4(0.f, 0.f, 0.f, -1.f);
    float comp = 0.f;
    if (p.mc[2] >= near_plane && p.mc[2] <= far_plane) {
      p.covar = quat_scale_to_covar(q, s);
      p.covar_c = mul_bt(mul(cam.R, p.covar), cam.R);
      persp_mid(cam, W, H, p);
      float a, b, c;
      cov2d_from(p.J, p.covar_c, a, b, c);
      float det_orig = a * c - b * b;
      a += eps2d;
      c += eps2d;
      float det = a * c - b * b;
      if (det > 0.f) {
        float bb = 0.5f * (a + c);
        float v1 = bb + sqrtf(fmaxf(0.01f, bb * bb - det));
        float rad = ceilf(3.f * sqrtf(v1));
        float mx = cam.fx * p.mc[0] * p.rz + cam.cx;
        float my = cam.fy * p.mc[1] * p.rz + cam.cy;
        bool ok = rad > radius_clip;
        ok = ok && !(mx + rad <= 0.f || mx - rad >= (float)W || my + rad <= 0.f || my - rad >= (float)H);
        if (ok) {
          float inv = 1.f / det;
          radius = (int)rad;
          comp = sqrtf(fmaxf(0.f, det_orig / det));
          float op = op_in;
          if (antialiased) op *= comp;
          float ca = c * inv, cb = -b * inv, cc = a * inv;
          o0 = make_float4(mx, my, p.mc[2], op);
          o1 = make_float4(ca, cb, cc, cull_radius(ca, cb, cc, op));
        }
      }
    }
    radii[i] = radius;
    GSL_Q(Q0, i) = o0;
    GSL_Q(Q1, i) = o1;
    if (comps) comps[i] = comp;
    float c0 = 0.f, c1 = 0.f, c2 = 0.f;
    if (RGB) {
      if (sh_degree < 0) {
        c0 = shc[0]; c1 = shc[1]; c2 = shc[2];
      } else {
        if (radius > 0) {  // masks = radii > 0
          M3 Ri;
          float cp[3];
          cam_inverse(cam, Ri, cp);
          float x = p.mean[0] - cp[0], y = p.mean[1] - cp[1], z = p.mean[2] - cp[2];
          float inorm = rsqrtf(x * x + y * y + z * z);
          float Y[16];
          sh_basis(sh_degree, x * inorm, y * inorm, z * inorm, Y);
          int nK = (sh_degree + 1) * (sh_degree + 1);
          const float* cf = colors + (size_t)i * K_sh * 3;
#pragma unroll
          for (int k = 0; k < 4; ++k)
            if (k < nK) { c0 += Y[k] * shc[3 * k]; c1 += Y[k] * shc[3 * k + 1]; c2 += Y[k] * shc[3 * k + 2]; }
          for (int k = 4; k < nK; ++k) {
            c0 += Y[k] * cf[3 * k]; c1 += Y[k] * cf[3 * k + 1]; c2 += Y[k] * cf[3 * k + 2];
          }
        }
        c0 = fmaxf(c0 + 0.5f, 0.f); c1 = fmaxf(c1 + 0.5f, 0.f); c2 = fmaxf(c2 + 0.5f, 0.f);
      }
      if (!Qh) GSL_Q(Q2, i) = make_float4(c0, c1, c2, 0.f);  // (fp16 staging: the compositing kernels read the colour from Qh)
    }
    if (Qh) store_half_record(Qh, (size_t)i, o0, o1, make_float4(c0, c1, c2, 0.f));
    if (radius > 0) {
      strip_rect(o0.x, o0.y, radius, 16, tile_w, tile_h, ty0, ty1, xmin, ymin, xmax, ymax);
      key = ((uint64_t)__float_as_uint(o0.z) << 32) | (uint32_t)(order_ids ? order_ids[i] : i);
    }
    if (tiles_per_gauss) tiles_per_gauss[i] = (xmax - xmin) * (ymax - ymin);
  }
  {
    const bool has = (ymin < ymax) && (xmin < xmax);
    int lo = has ? ymin * tile_w + xmin - tbase : nst, hi = has ? (ymax - 1) * tile_w + (xmax - 1) - tbase : -1;
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
      lo = min(lo, __shfl_xor(lo, o, 64));
      hi = max(hi, __shfl_xor(hi, o, 64));
    }
    if ((threadIdx.x & 63) == 0 && hi >= 0) { atomicMin(&s_rng[0], lo); atomicMax(&s_rng[1], hi); }
  }
  for (int y = ymin; y < ymax; ++y)
    for (int x = xmin; x < xmax; ++x) atomicAdd(&s_hist[y * tile_w + x - tbase], 1);
  __syncthreads();
  const int k_lo = __builtin_amdgcn_readfirstlane(s_rng[0]), k_hi = __builtin_amdgcn_readfirstlane(s_rng[1]);
  if (!BINNED) {
    for (int k = k_lo + (int)threadIdx.x; k <= k_hi; k += GSL_BIN_THREADS) {
      int c = s_hist[k];
      if (c) atomicAdd(&tile_counts[tbase + k], c);
    }
    return;
  }
  // all of a thread's returning atomics are issued before the first result is consumed
  int res[GSL_MAX_STRIP_TILES / GSL_BIN_THREADS];
#pragma unroll
  for (int u = 0; u < GSL_MAX_STRIP_TILES / GSL_BIN_THREADS; ++u) {
    res[u] = 0;
    if (k_lo + u * GSL_BIN_THREADS <= k_hi) {  // (wave-uniform)
      int k = k_lo + (int)threadIdx.x + u * GSL_BIN_THREADS;
      int c = (k <= k_hi) ? s_hist[k] : 0;
      res[u] = c ? atomicAdd(&tile_counts[tbase + k], c) : 0;
    }
  }
#pragma unroll
  for (int u = 0; u < GSL_MAX_STRIP_TILES / GSL_BIN_THREADS; ++u) {
    if (k_lo + u * GSL_BIN_THREADS <= k_hi) {
      int k = k_lo + (int)threadIdx.x + u * GSL_BIN_THREADS;
      if (k <= k_hi && s_hist[k]) s_hist[k] = res[u];  // first slot of this workgroup's span; ranks count up from it
    }
  }
  __syncthreads();
  for (int y = ymin; y < ymax; ++y)
    for (int x = xmin; x < xmax; ++x) {
      int lt = y * tile_w + x - tbase;
      int slot = atomicAdd(&s_hist[lt], 1);
      if (slot < bin_cap) bins[(size_t)(tbase + lt) * (size_t)bin_cap + slot] = key;
    }
}

}  // namespace gsl

// ---------------------------------------------------------------------------------------------- C ABI
extern "C" size_t gsl_fused_ws_bytes(int N, int n_tiles) {
  size_t nb = ((size_t)(N > 0 ? N : 1) + 255) / 256;
  return gsl::fused_vm_rows_offset(n_tiles > 0 ? n_tiles : 1) + (nb + GSL_VM_STAGE_ROWS) * 16 * sizeof(float);
}

// where gsl_fused_project_bwd leaves the pose-gradient rows inside ws: ceil(N / 256) rows of 16 floats (15 used)
extern "C" const float* gsl_fused_viewmat_rows(const void* ws, int n_tiles) {
  if (!ws || n_tiles <= 0) return nullptr;
  return (const float*)((const char*)ws + gsl::fused_vm_rows_offset(n_tiles));
}

extern "C" int gsl_fused_project(const float* means, const float* quats, const float* scales, const float* opacities,
                                 const float* colors, int sh_degree, int K_sh, const float* viewmat, const float* K,
                                 int N, int width, int height, float eps2d, float near_plane, float far_plane,
                                 float radius_clip, int antialiased, int tile_w, int tile_h, int ty0, int ty1,
                                 int32_t* radii, float* Q0, float* Q1, float* Q2, float* compensations,
                                 int32_t* tiles_per_gauss, int32_t* tile_offsets, int32_t* n_isects, void* ws,
                                 size_t ws_bytes, void* Qh, void* bins, int bin_cap, int32_t* flags,
                                 const int32_t* order_ids, void* stream) {
  if (N < 0 || width <= 0 || height <= 0 || tile_w <= 0 || tile_h <= 0 || ty0 < 0 || ty1 > tile_h || ty0 > ty1)
    return GSL_ERR_BAD_ARG;
  if (N > GSL_MAX_GAUSSIANS) return GSL_ERR_BAD_ARG;  // (packed gradient rows are addressed by 32-bit byte offsets)
  if (tile_w * 16 < width || tile_h * 16 < height) return GSL_ERR_BAD_ARG;
  int n_tiles = tile_w * tile_h, nst = (ty1 - ty0) * tile_w;
  if (nst > GSL_MAX_STRIP_TILES) return GSL_ERR_BAD_ARG;
  if (!viewmat || !K || !tile_offsets || !n_isects) return GSL_ERR_BAD_ARG;
  if (N > 0 && (!means || !quats || !scales || !opacities || !radii || !Q0 || !Q1)) return GSL_ERR_BAD_ARG;
  if (Q2 && !colors) return GSL_ERR_BAD_ARG;
  if (Q2 && sh_degree >= 0 && (sh_degree > 3 || K_sh < (sh_degree + 1) * (sh_degree + 1))) return GSL_ERR_BAD_ARG;
  if (antialiased && !compensations) return GSL_ERR_BAD_ARG;
  if (!ws || ws_bytes < gsl_fused_ws_bytes(N, n_tiles)) return GSL_ERR_WORKSPACE;
  if (bins && bin_cap <= 0) return GSL_ERR_BAD_ARG;
  hipStream_t st = (hipStream_t)stream;
  int32_t* counts = (int32_t*)ws;
  int32_t* cursors = counts + n_tiles;
  GSL_CLAMP_DEPTH_WINDOW(near_plane, far_plane);
  // binned mode relies on the scan leaving the counters cleared (ws zero-filled once by the caller): no clearing launch
  if (!bins && gsl::zero_u32(counts, (size_t)n_tiles, st) != GSL_OK) return GSL_ERR_HIP;
  if (N > 0) {
    dim3 grid((N + GSL_BIN_THREADS - 1) / GSL_BIN_THREADS), block(GSL_BIN_THREADS);
    size_t lds = (size_t)(nst + 2) * sizeof(int);  // counters + the touched range
#define CALL_P(RGBV, BINV)                                                                                            \
  hipLaunchKernelGGL((gsl::k_fproject<RGBV, BINV>), grid, block, lds, st, means, quats, scales, opacities, colors,    \
                     sh_degree, K_sh, viewmat, K, N, width, height, eps2d, near_plane, far_plane, radius_clip,        \
                     antialiased, tile_w, tile_h, ty0, ty1, radii, (float4*)Q0, (float4*)Q1, (float4*)Q2,             \
                     compensations, tiles_per_gauss, counts, (uint4*)Qh, (uint64_t*)bins, bin_cap,                   \
                     bins ? gsl::fused_bin_state(ws, n_tiles) : (int32_t*)nullptr, flags, order_ids)
    if (Q2) { if (bins) CALL_P(true, true); else CALL_P(true, false); }
    else { if (bins) CALL_P(false, true); else CALL_P(false, false); }
#undef CALL_P
    GSL_CHECK_LAUNCH();
  }
  if (bins) return GSL_OK;  // binned mode: gsl_fused_bin's sort kernel adds up the tile sizes itself
  gsl::launch_tile_scan(st, counts, n_tiles, tile_offsets, n_isects, cursors);
  GSL_CHECK_LAUNCH();
  return GSL_OK;
}

namespace gsl {
// gsl_fused_bin and gsl_fused_bin_clear (clear: the latter; rows: its N gradient rows, zeroed whichever way the call ends)
static int fused_bin(const float* Q0, const int32_t* radii, int N, int tile_w, int tile_h, int ty0, int ty1,
                     int32_t* tile_offsets, int64_t capacity, uint64_t* sort_keys, int32_t* flatten_ids,
                     int64_t* isect_ids, void* ws, size_t ws_bytes, int write_sorted_keys, void* bins, int bin_cap,
                     int32_t* n_isects, int32_t* flags, int long_min, const int32_t* order_ids,
                     const int32_t* storage_of, bool clear, float* rows, void* stream) {
  if (N < 0 || tile_w <= 0 || tile_h <= 0 || ty0 < 0 || ty1 > tile_h || ty0 > ty1 || capacity < 0)
    return GSL_ERR_BAD_ARG;
  if (clear && (N > GSL_MAX_GAUSSIANS || (N > 0 && !rows))) return GSL_ERR_BAD_ARG;
  if (!clear || N == 0) rows = nullptr;
  const int n_rows = rows ? N : 0;
  int n_tiles = tile_w * tile_h, nst = (ty1 - ty0) * tile_w;
  if (nst > GSL_MAX_STRIP_TILES || !tile_offsets) return GSL_ERR_BAD_ARG;
  if (bins) {
    // gsl_fused_project already put every key into its tile's bin and left the tile sizes in the counters: the sort
    // kernel runs over ALL tiles, writes tile_offsets[n_tiles + 1] and n_isects itself (sizes outside the strip are 0)
    if (bin_cap <= 0 || !n_isects) return GSL_ERR_BAD_ARG;
    if (!ws || ws_bytes < gsl_fused_ws_bytes(N, n_tiles)) return GSL_ERR_WORKSPACE;
    if (capacity > 0 && (!sort_keys || !flatten_ids)) return GSL_ERR_BAD_ARG;
    return gsl::tile_sort_keys(tile_offsets, 0, n_tiles, capacity, sort_keys, flatten_ids, isect_ids, 0,
                               write_sorted_keys, (uint64_t*)bins, bin_cap, (const int32_t*)ws, n_isects, flags,
                               write_sorted_keys ? 0 : long_min, nst, storage_of, rows, n_rows, stream);
  }
  if (N == 0 || capacity == 0 || nst == 0)  // no launch of the sort: the rows get one of their own
    return rows ? gsl::zero_u32(rows, (size_t)16 * (size_t)N, (hipStream_t)stream) : GSL_OK;
  if (!Q0 || !radii || !sort_keys || !flatten_ids) return GSL_ERR_BAD_ARG;
  if (!ws || ws_bytes < gsl_fused_ws_bytes(N, n_tiles)) return GSL_ERR_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  int32_t* cursors = (int32_t*)ws + n_tiles;
  gsl::launch_record_scatter(st, Q0, radii, order_ids, N, tile_w, tile_h, ty0, ty1, tile_offsets, cursors,
                             (long long)capacity, sort_keys);
  GSL_CHECK_LAUNCH();
  return gsl::tile_sort_keys(tile_offsets, ty0 * tile_w, nst, capacity, sort_keys, flatten_ids, isect_ids, 0,
                             write_sorted_keys, nullptr, 0, nullptr, nullptr, nullptr, 0, 0, storage_of, rows, n_rows,
                             stream);
}
}  // namespace gsl

extern "C" int gsl_fused_bin(const float* Q0, const int32_t* radii, int N, int tile_w, int tile_h, int ty0, int ty1,
                             int tile_n_bits, int32_t* tile_offsets, int64_t capacity, uint64_t* sort_keys,
                             int32_t* flatten_ids, int64_t* isect_ids, void* ws, size_t ws_bytes,
                             int write_sorted_keys, void* bins, int bin_cap, int32_t* n_isects, int32_t* flags,
                             int long_min, const int32_t* order_ids, const int32_t* storage_of, void* stream) {
  (void)tile_n_bits;
  return gsl::fused_bin(Q0, radii, N, tile_w, tile_h, ty0, ty1, tile_offsets, capacity, sort_keys, flatten_ids, isect_ids,
                        ws, ws_bytes, write_sorted_keys, bins, bin_cap, n_isects, flags, long_min, order_ids, storage_of,
                        false, nullptr, stream);
}

extern "C" int gsl_fused_bin_clear(const float* Q0, const int32_t* radii, int N, int tile_w, int tile_h, int ty0, int ty1,
                                   int tile_n_bits, int32_t* tile_offsets, int64_t capacity, uint64_t* sort_keys,
                                   int32_t* flatten_ids, int64_t* isect_ids, void* ws, size_t ws_bytes,
                                   int write_sorted_keys, void* bins, int bin_cap, int32_t* n_isects, int32_t* flags,
                                   int long_min, const int32_t* order_ids, const int32_t* storage_of, float* rows,
                                   void* stream) {
  (void)tile_n_bits;
  return gsl::fused_bin(Q0, radii, N, tile_w, tile_h, ty0, ty1, tile_offsets, capacity, sort_keys, flatten_ids, isect_ids,
                        ws, ws_bytes, write_sorted_keys, bins, bin_cap, n_isects, flags, long_min, order_ids, storage_of,
                        true, rows, stream);
}

extern "C" int gsl_fused_clear_rows(float* rows, int N, void* stream) {
  if (N < 0 || (N > 0 && !rows)) return GSL_ERR_BAD_ARG;
  return gsl::zero_u32(rows, (size_t)16 * (size_t)N, (hipStream_t)stream);
}
