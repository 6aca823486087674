// Shared device helpers for libgsloc_hip (gfx950 / CDNA4, wave64).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/gsloc_hip.h"

#define GSL_WAVE 64
#define GSL_ALPHA_MAX 0.999f
#define GSL_ALPHA_MIN (1.0f / 255.0f)
#define GSL_T_STOP 1e-4f
#define GSL_LOG2E 1.4426950408889634f

#define GSL_CHECK_LAUNCH()                                   \
  do {                                                       \
    hipError_t e__ = hipGetLastError();                      \
    if (e__ != hipSuccess) return GSL_ERR_HIP;               \
  } while (0)

namespace gsl {

struct M3 {  // row-major 3x3
  float m[9];
  __device__ __forceinline__ float& operator()(int r, int c) { return m[r * 3 + c]; }
  __device__ __forceinline__ float operator()(int r, int c) const { return m[r * 3 + c]; }
};

__device__ __forceinline__ M3 mul(const M3& a, const M3& b) {
  M3 o;
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j)
      o(i, j) = a(i, 0) * b(0, j) + a(i, 1) * b(1, j) + a(i, 2) * b(2, j);
  return o;
}
__device__ __forceinline__ M3 mul_bt(const M3& a, const M3& b) {  // a * b^T
  M3 o;
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j)
      o(i, j) = a(i, 0) * b(j, 0) + a(i, 1) * b(j, 1) + a(i, 2) * b(j, 2);
  return o;
}
__device__ __forceinline__ M3 mul_at(const M3& a, const M3& b) {  // a^T * b
  M3 o;
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j)
      o(i, j) = a(0, i) * b(0, j) + a(1, i) * b(1, j) + a(2, i) * b(2, j);
  return o;
}

// wxyz quaternion (normalised here) -> rotation matrix.
__device__ __forceinline__ M3 quat_to_rotmat(float w, float x, float y, float z) {
  float inv = rsqrtf(w * w + x * x + y * y + z * z);
  w *= inv; x *= inv; y *= inv; z *= inv;
  M3 R;
  R(0, 0) = 1.f - 2.f * (y * y + z * z); R(0, 1) = 2.f * (x * y - w * z); R(0, 2) = 2.f * (x * z + w * y);
  R(1, 0) = 2.f * (x * y + w * z); R(1, 1) = 1.f - 2.f * (x * x + z * z); R(1, 2) = 2.f * (y * z - w * x);
  R(2, 0) = 2.f * (x * z - w * y); R(2, 1) = 2.f * (y * z + w * x); R(2, 2) = 1.f - 2.f * (x * x + y * y);
  return R;
}

// Sigma = (Rq S)(Rq S)^T
__device__ __forceinline__ M3 quat_scale_to_covar(const float q[4], const float s[3]) {
  M3 R = quat_to_rotmat(q[0], q[1], q[2], q[3]);
  M3 M;
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) M(i, j) = R(i, j) * s[j];
  return mul_bt(M, M);
}

struct Cam {  // wave-uniform camera constants (scalar registers)
  M3 R;
  float t[3];
  float fx, fy, cx, cy;
};

__device__ __forceinline__ Cam load_cam(const float* __restrict__ V, const float* __restrict__ K) {
  Cam c;
#pragma unroll
  for (int i = 0; i < 3; ++i) {
#pragma unroll
    for (int j = 0; j < 3; ++j) c.R(i, j) = V[i * 4 + j];
    c.t[i] = V[i * 4 + 3];
  }
  c.fx = K[0]; c.fy = K[4]; c.cx = K[2]; c.cy = K[5];
  return c;
}

// Per-Gaussian records Q0/Q1/Q2: three arrays of float4.  (Measured alternatives, profiles/r02_backward_ablation.txt:
// one interleaved array of 64-byte rows made the random-order forward 10 % faster and projection / binning slower,
// no net gain; a workgroup -> tile map that gives each XCD one contiguous span of tiles changed nothing.)
#define GSL_Q(arr, g) (arr)[(g)]
// Pixel groups of an 8x8 quadrant in the compositing backward (raster_g16.hip): 4 = the four 4x4 blocks (one DPP row
// of 16 lanes each), 8 = the eight 4x2 half blocks (8 lanes each).  The forward's hit list carries one bit per group
// above the entry's list index: (group bits) << GSL_HIT_SHIFT | index.
#ifndef GSL_NG
#define GSL_NG 4
#endif
#define GSL_HIT_SHIFT (32 - GSL_NG)
#define GSL_HIT_INDEX_MASK ((1u << GSL_HIT_SHIFT) - 1u)
// Depths that reach the sort keys are positive, finite, normal floats: the window [near_plane, far_plane] of a projection
// is clamped to [FLT_MIN, FLT_MAX] on the host (a Gaussian at z <= 0 has no perspective projection anyway; the reference
// calls with near_plane = 0.01).  The per-tile sorts compare keys as doubles on that ground (sort_dev.h cswap).
#define GSL_CLAMP_DEPTH_WINDOW(nearp, farp)            \
  do {                                                 \
    if (!((nearp) >= 1.17549435e-38f)) (nearp) = 1.17549435e-38f; \
    if (!((farp) <= 3.40282347e+38f)) (farp) = 3.40282347e+38f;   \
  } while (0)
// Most Gaussians one call takes: the compositing backward addresses a Gaussian's 64-byte gradient row by a 32-bit byte
// offset (id << 6).  2^26 Gaussians are 4 GiB of rows; the largest configuration of BASELINE.json has 5 M.
#define GSL_MAX_GAUSSIANS (1 << 26)
// Workgroup -> work item.  Workgroups go to the eight XCDs round-robin (workgroup b runs on XCD b % 8), and every XCD has
// its own 4 MiB L2.  With GSL_XCD_SPANS the items (tiles, in raster order) are dealt so that XCD x gets ONE contiguous
// span of them: with the Gaussians stored in tile order (context.py:_choose_placement) the records an XCD gathers are
// then one eighth of the frame's instead of all of them.  (Round 2 tried the same map on randomly ordered records: no
// locality to keep, no effect.)
#ifndef GSL_XCD_SPANS
#define GSL_XCD_SPANS 0
#endif
__device__ __forceinline__ int xcd_span_item(int b, int n) {
#if GSL_XCD_SPANS
  const int x = b & 7, k = b >> 3, q = n >> 3, r = n & 7;
  return x * q + min(x, r) + k;
#else
  (void)n;
  return b;
#endif
}
#define GSL_TILE_OF_BLOCK() gsl::xcd_span_item((int)blockIdx.x, (int)gridDim.x)

// ---- fp16-staged records (workload X, "fp16 compositing": BASELINE.json configs[4]) --------------------
// One 32-byte record per Gaussian for the compositing kernels instead of three 16-byte ones: the centre stays float32
// (a 1920-px coordinate needs it) and so is the depth feature (a camera-space depth reaches far_plane = 1e10, the half
// range ends at 65504); conic, cull radius, opacity and colour are halves.  Everything the compositing loops accumulate
// (T, colour sums, gradient sums) stays float32: the records are widened when they are staged in LDS, so the loops
// themselves are the float32 ones.
//   dw0 x   dw1 y   dw2 (conic a | b)   dw3 (conic c | r_cull, rounded up)   dw4 (0 | opacity)   dw5 (r | g)   dw6 (b | 0)
//   dw7 depth feature (float32)
// Half range: conic entries are at most 1/eps2d (RenderContext refuses fp16 staging below eps2d = 2e-5); opacities lie in
// [0, 1]; colours (after SH and the clamp at 0) are finite up to 65504 and become +inf above, with 11 significant bits.
__device__ __forceinline__ unsigned pack2h(float a, float b) {
  _Float16 ha = (_Float16)a, hb = (_Float16)b;
  return (unsigned)__builtin_bit_cast(unsigned short, ha) | ((unsigned)__builtin_bit_cast(unsigned short, hb) << 16);
}
__device__ __forceinline__ float h_lo(unsigned u) { return (float)__builtin_bit_cast(_Float16, (unsigned short)(u & 0xFFFFu)); }
__device__ __forceinline__ float h_hi(unsigned u) { return (float)__builtin_bit_cast(_Float16, (unsigned short)(u >> 16)); }

__device__ __forceinline__ void store_half_record(uint4* __restrict__ Qh, size_t i, float4 q0, float4 q1, float4 q2) {
  float rc = (q1.w > 0.f && q1.w < 6.0e4f) ? q1.w * 1.002f + 0.01f : q1.w;  // conservative radius: never rounded down
  Qh[2 * i] = make_uint4(__float_as_uint(q0.x), __float_as_uint(q0.y), pack2h(q1.x, q1.y), pack2h(q1.z, rc));
  Qh[2 * i + 1] = make_uint4(pack2h(0.f, q0.w), pack2h(q2.x, q2.y), pack2h(q2.z, 0.f), __float_as_uint(q0.z));
}

// Record g for the compositing kernels: the float32 arrays, or the fp16-staged array when Qh is given.
__device__ __forceinline__ void load_record(const float4* __restrict__ Q0, const float4* __restrict__ Q1,
                                            const float4* __restrict__ Q2, const uint4* __restrict__ Qh, int g,
                                            bool want_rgb, float4& r0, float4& r1, float4& r2) {
  if (Qh) {
    uint4 lo = Qh[2 * (size_t)g], hi = Qh[2 * (size_t)g + 1];
    r0 = make_float4(__uint_as_float(lo.x), __uint_as_float(lo.y), __uint_as_float(hi.w), h_hi(hi.x));
    r1 = make_float4(h_lo(lo.z), h_hi(lo.z), h_lo(lo.w), h_hi(lo.w));
    r2 = make_float4(h_lo(hi.y), h_hi(hi.y), h_lo(hi.z), 0.f);
  } else {
    r0 = GSL_Q(Q0, g);
    r1 = GSL_Q(Q1, g);
    if (want_rgb) r2 = GSL_Q(Q2, g);
  }
}

// Tile-order placement of the Gaussians (RenderContext(reorder=True)): the caller stores its Gaussians
// sorted by the tile of their centre, once per frame, so that the record gathers of a tile's list fall on a few contiguous
// runs.  The list ORDER must not change with the placement -- depth ties break by Gaussian index -- so the
// low key word stays the Gaussian's ORIGINAL index (order_ids[storage slot], given to the projection) and the sorts translate
// it to the storage slot (storage_of[original index]) only when they write the list.  Both NULL: identity.
__device__ __forceinline__ int32_t list_id(const int32_t* __restrict__ storage_of, uint64_t key) {
  uint32_t g = (uint32_t)key;
  return storage_of ? storage_of[g] : (int32_t)g;
}

// DPP lane exchange (no LDS traffic).  Lanes a row_mask disables contribute 0.
template <int CTRL, int ROW_MASK = 0xF>
__device__ __forceinline__ float dpp_get(float v) {
  return __builtin_bit_cast(
      float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, ROW_MASK, 0xF, true));
}

// LDS written by some lanes of a wave is read by other lanes of the same wave: orders the accesses without a barrier.
__device__ __forceinline__ void wave_lds_fence() {
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

// Sum over the 64 lanes of a wave in 6 DPP adds (quad swaps, row mirrors, row broadcasts);
// the total comes back wave-uniform (scalar register) from lane 63.  Fixed order => deterministic.
__device__ __forceinline__ float wave_sum(float v) {
  v += dpp_get<0xB1>(v);        // quad_perm [1,0,3,2]
  v += dpp_get<0x4E>(v);        // quad_perm [2,3,0,1]
  v += dpp_get<0x141>(v);       // row_half_mirror
  v += dpp_get<0x140>(v);       // row_mirror: every lane holds its 16-lane row sum
  v += dpp_get<0x142, 0xA>(v);  // row_bcast15 into rows 1,3
  v += dpp_get<0x143, 0xC>(v);  // row_bcast31 into rows 2,3
  return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), 63));
}

// Lane select driven by a 64-bit scalar mask: t in the lanes of m, f elsewhere (v_cndmask_b32_e64 with an SGPR pair).
// Measured on MI355X: the VOP2 form that reads VCC issues ~5x slower than this form (9.5 vs 1.8 ns per
// wave-instruction per SIMD), and hipcc picks the VCC form for plain ?: selects -- so the hot loops keep their
// predicates as scalar masks (__ballot, lane-constant literals) and select through this helper.
#define GSL_SEL_ASM(r, m, t, f) asm("v_cndmask_b32_e64 %0, %1, %2, %3" : "=v"(r) : "v"(f), "v"(t), "s"(m))
__device__ __forceinline__ float sel(unsigned long long m, float t, float f) { float r; GSL_SEL_ASM(r, m, t, f); return r; }
__device__ __forceinline__ unsigned sel(unsigned long long m, unsigned t, unsigned f) { unsigned r; GSL_SEL_ASM(r, m, t, f); return r; }
__device__ __forceinline__ int sel(unsigned long long m, int t, int f) { int r; GSL_SEL_ASM(r, m, t, f); return r; }

// Expected depth ("ED"): the forward divides the depth channel's sum by the pixel's alpha, guarded at GSL_ED_ALPHA_MIN.
// The backward kernels undo that once per pixel, before the walk: vd (upstream gradient of the expected depth dn)
// becomes the gradient of the depth sum, vd / alpha, and the alpha gradient gains -vd dn / alpha.
#define GSL_ED_ALPHA_MIN 1e-10f
struct EdGrad { float va, vd; };
__device__ __forceinline__ EdGrad ed_backward(float Aimg, float dn, float va, float vd) {
  if (Aimg >= GSL_ED_ALPHA_MIN) va += -vd * dn / Aimg;
  return {va, vd / fmaxf(Aimg, GSL_ED_ALPHA_MIN)};
}

// Inverse of the rotation block and the camera position -R^-1 t (what torch.inverse(viewmat)[:3,3] is).
__device__ __forceinline__ void cam_inverse(const Cam& cam, M3& Ri, float cp[3]) {
  const M3& R = cam.R;
  float c00 = R(1, 1) * R(2, 2) - R(1, 2) * R(2, 1);
  float c01 = R(1, 2) * R(2, 0) - R(1, 0) * R(2, 2);
  float c02 = R(1, 0) * R(2, 1) - R(1, 1) * R(2, 0);
  float det = R(0, 0) * c00 + R(0, 1) * c01 + R(0, 2) * c02;
  float id = 1.f / det;
  Ri(0, 0) = c00 * id; Ri(1, 0) = c01 * id; Ri(2, 0) = c02 * id;
  Ri(0, 1) = (R(0, 2) * R(2, 1) - R(0, 1) * R(2, 2)) * id;
  Ri(1, 1) = (R(0, 0) * R(2, 2) - R(0, 2) * R(2, 0)) * id;
  Ri(2, 1) = (R(0, 1) * R(2, 0) - R(0, 0) * R(2, 1)) * id;
  Ri(0, 2) = (R(0, 1) * R(1, 2) - R(0, 2) * R(1, 1)) * id;
  Ri(1, 2) = (R(0, 2) * R(1, 0) - R(0, 0) * R(1, 2)) * id;
  Ri(2, 2) = (R(0, 0) * R(1, 1) - R(0, 1) * R(1, 0)) * id;
#pragma unroll
  for (int k = 0; k < 3; ++k) cp[k] = -(Ri(k, 0) * cam.t[0] + Ri(k, 1) * cam.t[1] + Ri(k, 2) * cam.t[2]);
}

}  // namespace gsl

