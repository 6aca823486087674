// Projection backward of the fused pipeline: per-Gaussian vjp of projection + colour from the compositing backward's
// gradient rows (k_fproject_bwd, with pass 2 of the tiny-splat backward and the deterministic row gather fused in), and
// the fixed-order reduction of the pose gradient (k_freduce_rows, k_freduce_viewmat).
#include "gsloc_internal.h"
#include "pose_dev.h"
#include "project_dev.h"
#include "sh_dev.h"
#include "tile_dev.h"
#include "tiny_dev.h"

namespace gsl {

// ------------------------------------------------------------------------------------------------
// Backward 2: per-Gaussian vjp of projection + colour, and the pose reduction.
// Reads (and clears) the 64-byte gradient rows.  partial rows: [v_R 9][v_t 3][v_campos 3].
// KEEP (gsl_fused_project_bwd_keep, general path only): the rows are read and left as they are -- the sort launch of
// the next forward clears them (gsl_fused_bin_clear), and this kernel, which runs at what the memory system gives,
// writes 48 bytes of zeros per Gaussian less.
// ------------------------------------------------------------------------------------------------
template <bool FULL, int D, bool KEEP>
__global__ __launch_bounds__(256) void k_fproject_bwd(
    const float* __restrict__ means, const float* __restrict__ quats, const float* __restrict__ scales,
    const float* __restrict__ opacities, const float* __restrict__ colors, int sh_degree, int K_sh,
    const float* __restrict__ V, const float* __restrict__ Kmat, int N, int W, int H, float eps2d, int antialiased,
    const int32_t* __restrict__ radii, const float4* __restrict__ Q1, const float* __restrict__ comps,
    float4* __restrict__ vacc, float* __restrict__ v_means, float* __restrict__ v_quats,
    float* __restrict__ v_scales, float* __restrict__ v_opacities, float* __restrict__ v_colors,
    float* __restrict__ partials, const float4* __restrict__ vrow, const uint64_t* __restrict__ skeys,
    const int32_t* __restrict__ tile_offsets, const float4* __restrict__ Q0, int tile_w, int tile_h, int ty0, int ty1,
    long long capacity, float4* __restrict__ trec, const float* __restrict__ vcT, int32_t* __restrict__ vc_state) {
  constexpr bool RGB = D >= 3;
  int i = blockIdx.x * 256 + threadIdx.x;
  Cam cam = load_cam(V, Kmat);
  // vc_state (may be NULL): 1 = the caller's v_colors buffer is known to hold zeros only (it is the same buffer call after
  // call, and nobody has written a non-zero since); a Gaussian without a colour gradient -- every Gaussian, under
  // GsplatLoc's depth-only loss -- then skips its 48 bytes of zero stores.  A thread that writes a real gradient marks
  // the buffer dirty (2); k_freduce_viewmat, which runs after the whole grid, turns "nobody wrote a non-zero in a launch
  // that stored everything" into 1 again.
  const bool vc_zero = FULL && RGB && vc_state && *vc_state == 1;
  // tiny-splat backward, pass 2 fused in: four lanes per Gaussian fold its 4x4 slab of (w, alpha*T) records into the
  // gradient row, which stays in LDS for the thread that owns the Gaussian (no row round trip, no gather launch)
  __shared__ float4 srow[256][3];
  if (trec) {
#pragma unroll 1
    for (int half = 0; half < 2; ++half) {  // two (Gaussian, slab row) items per turn: their loads leave together
      TinySlabIn in[2];
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        int t = (2 * half + u) * 256 + threadIdx.x;
        in[u] = tiny_slab_load(radii, Q0, Q1, trec, blockIdx.x * 256 + (t >> 2), t & 3, N);
      }
      GSL_TINY_SLAB_PIN(in[0]);
      GSL_TINY_SLAB_PIN(in[1]);
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        int t = (2 * half + u) * 256 + threadIdx.x;
        int lg = t >> 2, r = t & 3, gid = blockIdx.x * 256 + lg;
        float v[6 + D];
        tiny_slab_fold<D>(in[u], W, H, trec, vcT, gid, r, v);
        float pad[12];
#pragma unroll
        for (int k = 0; k < 12; ++k) pad[k] = (k < 6 + D) ? v[k] : 0.f;
        if (r == 0) srow[lg][0] = make_float4(pad[0], pad[1], pad[2], pad[3]);
        if (r == 1) srow[lg][1] = make_float4(pad[4], pad[5], pad[6], pad[7]);
        if (r == 2) srow[lg][2] = make_float4(pad[8], pad[9], pad[10], pad[11]);
      }
    }
    __syncthreads();
  }
  float acc15[15];
#pragma unroll
  for (int k = 0; k < 15; ++k) acc15[k] = 0.f;
  float vmean[3] = {0.f, 0.f, 0.f}, vq[4] = {0.f, 0.f, 0.f, 0.f}, vs[3] = {0.f, 0.f, 0.f};
  float vop = 0.f;
  float vrgb[3] = {0.f, 0.f, 0.f};
  bool live = (i < N) && (radii[i] > 0);
  bool sh_live = false;
  if (live) {
    float4 r0, r1, r2;
    float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
    if (vrow) {
      // deterministic mode: the Gaussian's rows were stored per intersection; find its entry in each tile list of
      // its rectangle (the lists are sorted by (depth bits, id): binary search) and add the rows in tile order
      r0 = r1 = r2 = z;
      float4 q0 = GSL_Q(Q0, i);
      int xmin, ymin, xmax, ymax;
      tile_rect(q0.x, q0.y, radii[i], 16, tile_w, tile_h, xmin, ymin, xmax, ymax);
      ymin = max(ymin, ty0);
      ymax = min(ymax, ty1);
      uint64_t want = ((uint64_t)__float_as_uint(q0.z) << 32) | (uint32_t)i;
      for (int y = ymin; y < ymax; ++y)
        for (int x = xmin; x < xmax; ++x) {
          long long lo = tile_offsets[y * tile_w + x], hi = tile_offsets[y * tile_w + x + 1];
          if (hi > capacity) hi = capacity;
          while (lo < hi) {
            long long mid = (lo + hi) >> 1;
            if (skeys[mid] < want) lo = mid + 1; else hi = mid;
          }
          if (lo < capacity && skeys[lo] == want) {
            float4 a = vrow[4 * lo], b = vrow[4 * lo + 1], c = vrow[4 * lo + 2];
            r0.x += a.x; r0.y += a.y; r0.z += a.z; r0.w += a.w;
            r1.x += b.x; r1.y += b.y; r1.z += b.z; r1.w += b.w;
            r2.x += c.x; r2.y += c.y; r2.z += c.z; r2.w += c.w;
          }
        }
    } else if (trec) {
      r0 = srow[threadIdx.x][0]; r1 = srow[threadIdx.x][1]; r2 = srow[threadIdx.x][2];
      if (vacc) {  // tiny-splat mode with long tile lists: those tiles' rows arrive through vacc (gsl_long_raster_bwd)
        float4 a = vacc[4 * (size_t)i], b = vacc[4 * (size_t)i + 1], c = vacc[4 * (size_t)i + 2];
        if (a.x != 0.f || a.y != 0.f || a.z != 0.f || a.w != 0.f || b.x != 0.f || b.y != 0.f || b.z != 0.f || b.w != 0.f ||
            c.x != 0.f || c.y != 0.f || c.z != 0.f || c.w != 0.f) {
          r0.x += a.x; r0.y += a.y; r0.z += a.z; r0.w += a.w;
          r1.x += b.x; r1.y += b.y; r1.z += b.z; r1.w += b.w;
          r2.x += c.x; r2.y += c.y; r2.z += c.z; r2.w += c.w;
          vacc[4 * (size_t)i] = z; vacc[4 * (size_t)i + 1] = z; vacc[4 * (size_t)i + 2] = z;
        }
      }
    } else {
      r0 = vacc[4 * (size_t)i]; r1 = vacc[4 * (size_t)i + 1]; r2 = vacc[4 * (size_t)i + 2];
      if (!KEEP) { vacc[4 * (size_t)i] = z; vacc[4 * (size_t)i + 1] = z; vacc[4 * (size_t)i + 2] = z; }
    }
    // row = [vx vy | va vb vc | vop | col0 col1 col2 col3 ...]
    float vm2x = r0.x, vm2y = r0.y, v_ca = r0.z, v_cb = r0.w, v_cc = r1.x, vop_eff = r1.y;
    float col[4] = {r1.z, r1.w, r2.x, r2.y};
    float vdepth = (D == 1) ? col[0] : ((D == 4) ? col[3] : 0.f);
    if (RGB) { vrgb[0] = col[0]; vrgb[1] = col[1]; vrgb[2] = col[2]; }
    float comp = 0.f, vcomp = 0.f;
    vop = vop_eff;
    if (antialiased) {
      comp = comps[i];
      vcomp = vop_eff * opacities[i];
      vop = vop_eff * comp;
    }
    ProjMid p;
    float q[4], s[3];
    load_gaussian(means, quats, scales, i, cam, p, q, s);
    p.covar = quat_scale_to_covar(q, s);
    p.covar_c = mul_bt(mul(cam.R, p.covar), cam.R);
    persp_mid(cam, W, H, p);
    float4 q1 = GSL_Q(Q1, i);
    project_vjp<FULL>(cam, eps2d, p, q, s, q1.x, q1.y, q1.z, vm2x, vm2y, vdepth, v_ca, v_cb, v_cc, antialiased != 0,
                      comp, vcomp, acc15, vmean, vq, vs);
    sh_live = RGB && (sh_degree >= 0) && (vrgb[0] != 0.f || vrgb[1] != 0.f || vrgb[2] != 0.f);
    if (sh_live) {
      // colour = max(SH(dir) + 0.5, 0), dir = mean - campos
      M3 Ri;
      float cp[3];
      cam_inverse(cam, Ri, cp);
      float rx = p.mean[0] - cp[0], ry = p.mean[1] - cp[1], rz = p.mean[2] - cp[2];
      float inorm = rsqrtf(rx * rx + ry * ry + rz * rz);
      float x = rx * inorm, y = ry * inorm, zz = rz * inorm;
      float Y[16];
      sh_basis(sh_degree, x, y, zz, Y);
      int nK = (sh_degree + 1) * (sh_degree + 1);
      const float* cf = colors + (size_t)i * K_sh * 3;
      float c0 = 0.5f, c1 = 0.5f, c2 = 0.5f;
      for (int k = 0; k < nK; ++k) {
        c0 += Y[k] * cf[3 * k]; c1 += Y[k] * cf[3 * k + 1]; c2 += Y[k] * cf[3 * k + 2];
      }
      if (!(c0 > 0.f)) vrgb[0] = 0.f;  // clamp_min(x, 0) passes the gradient where x > 0
      if (!(c1 > 0.f)) vrgb[1] = 0.f;
      if (!(c2 > 0.f)) vrgb[2] = 0.f;
      float sk[16];
      for (int k = 0; k < nK; ++k) {
        sk[k] = cf[3 * k] * vrgb[0] + cf[3 * k + 1] * vrgb[1] + cf[3 * k + 2] * vrgb[2];
        if (FULL) {
          if (k == 0 && vc_state) *vc_state = 2;
          v_colors[((size_t)i * K_sh + k) * 3] = Y[k] * vrgb[0];
          v_colors[((size_t)i * K_sh + k) * 3 + 1] = Y[k] * vrgb[1];
          v_colors[((size_t)i * K_sh + k) * 3 + 2] = Y[k] * vrgb[2];
        }
      }
      if (FULL)
        for (int k = nK * 3; k < K_sh * 3; ++k) v_colors[(size_t)i * K_sh * 3 + k] = 0.f;
      float g[3];
      sh_basis_grad(sh_degree, x, y, zz, sk, g);
      float dd = g[0] * x + g[1] * y + g[2] * zz;
      float gd[3] = {(g[0] - dd * x) * inorm, (g[1] - dd * y) * inorm, (g[2] - dd * zz) * inorm};
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        vmean[k] += gd[k];
        acc15[12 + k] = -gd[k];
      }
    }
  }
  if (FULL && i < N) {
#pragma unroll
    for (int k = 0; k < 3; ++k) v_means[3 * (size_t)i + k] = vmean[k];
#pragma unroll
    for (int k = 0; k < 4; ++k) v_quats[4 * (size_t)i + k] = vq[k];
#pragma unroll
    for (int k = 0; k < 3; ++k) v_scales[3 * (size_t)i + k] = vs[k];
    v_opacities[i] = vop;
    if (RGB && !sh_live) {
      if (sh_degree < 0) {
        const bool nz = vrgb[0] != 0.f || vrgb[1] != 0.f || vrgb[2] != 0.f;
        if (nz && vc_state) *vc_state = 2;
        if (nz || !vc_zero) {
          v_colors[3 * (size_t)i] = vrgb[0]; v_colors[3 * (size_t)i + 1] = vrgb[1]; v_colors[3 * (size_t)i + 2] = vrgb[2];
        }
      } else if (!vc_zero) {
        // (12 coefficients = 48 bytes per Gaussian for SH degree 1: three 16-byte stores instead of twelve strided
        // 4-byte ones; any other band count keeps the loop)
        if (K_sh == 4) {
          float4* dst = reinterpret_cast<float4*>(v_colors + (size_t)i * 12);
          float4 z4 = make_float4(0.f, 0.f, 0.f, 0.f);
          dst[0] = z4; dst[1] = z4; dst[2] = z4;
        } else {
          for (int k = 0; k < K_sh * 3; ++k) v_colors[(size_t)i * K_sh * 3 + k] = 0.f;
        }
      }
    }
  }
  if (partials != nullptr) {
    __shared__ float red[4][15];
    int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < 15; ++k) {
      float sum = wave_sum(acc15[k]);
      if (lane == 0) red[wv][k] = sum;
    }
    __syncthreads();
    if (threadIdx.x < 15)
      partials[(size_t)blockIdx.x * 16 + threadIdx.x] =
          red[0][threadIdx.x] + red[1][threadIdx.x] + red[2][threadIdx.x] + red[3][threadIdx.x];
  }
}

// Fixed-order sum of the partial rows, chain of the SH view direction through the camera
// position (campos = -R^-1 t), result into v_viewmat[16] (row 3 = 0: that row is constant).
// Stage 1 for many rows (N > 1 M: one workgroup summing 19 532 rows took 41 us at workload X): 64 workgroups each add
// up a contiguous span of rows (same thread layout as reduce_viewmat_rows: thread = (row mod 64, quarter), fixed order)
// into one row of `out`; k_freduce_viewmat then sums those 64.
__global__ __launch_bounds__(256) void k_freduce_rows(const float* __restrict__ partials, int nb, float* __restrict__ out) {
  __shared__ float red[4][16];
  int span = (nb + (int)gridDim.x - 1) / (int)gridDim.x;
  int r0 = blockIdx.x * span, r1 = min(nb, r0 + span);
  int q = threadIdx.x & 3;
  const float4* rows = reinterpret_cast<const float4*>(partials) + q;
  float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int b = r0 + (threadIdx.x >> 2); b < r1; b += 64) {
    float4 x = rows[(size_t)b * 4];
    a.x += x.x; a.y += x.y; a.z += x.z; a.w += x.w;
  }
  float v4[4] = {a.x, a.y, a.z, a.w};
  int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    float x = v4[c];
#pragma unroll
    for (int o = 4; o < 64; o <<= 1) x += __shfl_xor(x, o, 64);
    if (lane < 4) red[wv][4 * q + c] = x;
  }
  __syncthreads();
  if (threadIdx.x < 16)
    out[(size_t)blockIdx.x * 16 + threadIdx.x] =
        threadIdx.x < 15 ? (red[0][threadIdx.x] + red[1][threadIdx.x]) + (red[2][threadIdx.x] + red[3][threadIdx.x]) : 0.f;
}

__global__ __launch_bounds__(1024) void k_freduce_viewmat(const float* __restrict__ partials, int nb,
                                                         const float* __restrict__ V, const float* __restrict__ Kmat,
                                                         float* __restrict__ v_viewmat, int32_t* __restrict__ vc_state) {
  __shared__ float red[16][15];
  __shared__ float tot[15];
  float v = reduce_viewmat_rows_wide(partials, nb, V, Kmat, red, tot);
  if (threadIdx.x < 16) v_viewmat[threadIdx.x] = v;
  // (see k_fproject_bwd) 2: a real colour gradient was written in the launch before this one -> unknown; otherwise every
  // Gaussian's slot holds zeros now
  if (vc_state && threadIdx.x == 0) *vc_state = (*vc_state == 2) ? 0 : 1;
}

// gsl_fused_project_bwd and gsl_fused_project_bwd_keep (keep: the latter -- the rows of vacc, which it must be given
// and which are the only source it takes, are left as read)
static int fused_project_bwd(const float* means, const float* quats, const float* scales, const float* opacities,
                             const float* colors, int sh_degree, int K_sh, const float* viewmat, const float* K, int N,
                             int width, int height, float eps2d, int antialiased, int channels, const int32_t* radii,
                             const float* Q1, const float* compensations, float* vacc, float* v_means, float* v_quats,
                             float* v_scales, float* v_opacities, float* v_colors, float* v_viewmat, void* ws,
                             size_t ws_bytes, int n_tiles, const float* vrow, const uint64_t* sorted_keys,
                             const int32_t* tile_offsets, const float* Q0, int tile_w, int tile_h, int ty0, int ty1,
                             int64_t capacity, float* tiny_trec, const float* tiny_vcT, int reduce_viewmat,
                             int32_t* v_colors_state, bool keep, void* stream) {
  if (N < 0 || width <= 0 || height <= 0 || n_tiles <= 0) return GSL_ERR_BAD_ARG;
  if (keep && (vrow || tiny_trec || (N > 0 && !vacc))) return GSL_ERR_BAD_ARG;
  if (reduce_viewmat && !v_viewmat) return GSL_ERR_BAD_ARG;
  if (channels != 1 && channels != 3 && channels != 4) return GSL_ERR_BAD_ARG;
  bool full = v_means != nullptr;
  if (full != (v_quats != nullptr) || full != (v_scales != nullptr) || full != (v_opacities != nullptr))
    return GSL_ERR_BAD_ARG;
  if (full && channels >= 3 && !v_colors) return GSL_ERR_BAD_ARG;
  if (antialiased && !compensations) return GSL_ERR_BAD_ARG;
  hipStream_t st = (hipStream_t)stream;
  if (N == 0) {
    if (reduce_viewmat && gsl::zero_u32(v_viewmat, 16, st) != GSL_OK) return GSL_ERR_HIP;
    return GSL_OK;
  }
  if (!means || !quats || !scales || !opacities || !viewmat || !K || !radii || !Q1) return GSL_ERR_BAD_ARG;
  if (!vrow && !vacc && !tiny_trec) return GSL_ERR_BAD_ARG;
  if (tiny_trec && (!tiny_vcT || !Q0 || vrow)) return GSL_ERR_BAD_ARG;
  if (vrow && (!sorted_keys || !tile_offsets || !Q0 || tile_w <= 0 || tile_h <= 0 || tile_w * tile_h != n_tiles ||
               ty0 < 0 || ty1 > tile_h || ty0 > ty1 || capacity < 0))
    return GSL_ERR_BAD_ARG;
  if (channels >= 3 && !colors) return GSL_ERR_BAD_ARG;
  if (!ws || ws_bytes < gsl_fused_ws_bytes(N, n_tiles)) return GSL_ERR_WORKSPACE;
  // one row of 15 sums per workgroup; reduce_viewmat = 0 leaves them for gsl_pose_step / gsl_pack_pose_reduce
  float* partials = (float*)((char*)ws + gsl::fused_vm_rows_offset(n_tiles));
  int grid = (N + 255) / 256;
  int32_t* vcs = (full && channels >= 3) ? v_colors_state : nullptr;
#define CALL_PB(FF, DD)                                                                                               \
  do {                                                                                                                \
    auto kern = keep ? gsl::k_fproject_bwd<FF, DD, true> : gsl::k_fproject_bwd<FF, DD, false>;                        \
    hipLaunchKernelGGL(kern, dim3(grid), dim3(256), 0, st, means, quats, scales, opacities, colors, sh_degree, K_sh,  \
                       viewmat, K, N, width, height, eps2d, antialiased, radii, (const float4*)Q1, compensations,     \
                       (float4*)vacc, v_means, v_quats, v_scales, v_opacities, v_colors, partials,                    \
                       (const float4*)vrow, sorted_keys, tile_offsets, (const float4*)Q0, tile_w, tile_h, ty0, ty1,   \
                       (long long)capacity, (float4*)tiny_trec, tiny_vcT, vcs);                                       \
  } while (0)
  if (full) {
    if (channels == 1) CALL_PB(true, 1); else if (channels == 3) CALL_PB(true, 3); else CALL_PB(true, 4);
  } else {
    if (channels == 1) CALL_PB(false, 1); else if (channels == 3) CALL_PB(false, 3); else CALL_PB(false, 4);
  }
#undef CALL_PB
  GSL_CHECK_LAUNCH();
  if (reduce_viewmat) {
    if (grid > 8192) {  // two stages (fixed order either way)
      float* stage = partials + (size_t)grid * 16;
      hipLaunchKernelGGL(gsl::k_freduce_rows, dim3(GSL_VM_STAGE_ROWS), dim3(256), 0, st, partials, grid, stage);
      hipLaunchKernelGGL(gsl::k_freduce_viewmat, dim3(1), dim3(1024), 0, st, stage, GSL_VM_STAGE_ROWS, viewmat, K, v_viewmat, vcs);
    } else {
      hipLaunchKernelGGL(gsl::k_freduce_viewmat, dim3(1), dim3(1024), 0, st, partials, grid, viewmat, K, v_viewmat, vcs);
    }
    GSL_CHECK_LAUNCH();
  }
  return GSL_OK;
}
}  // namespace gsl

#define GSL_PROJECT_BWD_PARAMS                                                                                         \
  const float *means, const float *quats, const float *scales, const float *opacities, const float *colors,           \
      int sh_degree, int K_sh, const float *viewmat, const float *K, int N, int width, int height, float eps2d,       \
      int antialiased, int channels, const int32_t *radii, const float *Q1, const float *compensations, float *vacc,  \
      float *v_means, float *v_quats, float *v_scales, float *v_opacities, float *v_colors, float *v_viewmat,         \
      void *ws, size_t ws_bytes, int n_tiles, const float *vrow, const uint64_t *sorted_keys,                         \
      const int32_t *tile_offsets, const float *Q0, int tile_w, int tile_h, int ty0, int ty1, int64_t capacity,       \
      float *tiny_trec, const float *tiny_vcT, int reduce_viewmat, int32_t *v_colors_state, void *stream
#define GSL_PROJECT_BWD_ARGS(KEEP)                                                                                    \
  means, quats, scales, opacities, colors, sh_degree, K_sh, viewmat, K, N, width, height, eps2d, antialiased,         \
      channels, radii, Q1, compensations, vacc, v_means, v_quats, v_scales, v_opacities, v_colors, v_viewmat, ws,     \
      ws_bytes, n_tiles, vrow, sorted_keys, tile_offsets, Q0, tile_w, tile_h, ty0, ty1, capacity, tiny_trec,          \
      tiny_vcT, reduce_viewmat, v_colors_state, KEEP, stream
extern "C" int gsl_fused_project_bwd(GSL_PROJECT_BWD_PARAMS) {
  return gsl::fused_project_bwd(GSL_PROJECT_BWD_ARGS(false));
}
extern "C" int gsl_fused_project_bwd_keep(GSL_PROJECT_BWD_PARAMS) {
  return gsl::fused_project_bwd(GSL_PROJECT_BWD_ARGS(true));
}
#undef GSL_PROJECT_BWD_PARAMS
#undef GSL_PROJECT_BWD_ARGS
