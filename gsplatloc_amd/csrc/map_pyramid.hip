// Frame-to-map localisation: the image pyramid of a frame (gsplatloc_amd/mapping.py: GaussianMap.pyramid and the
// levels= argument of align_pose, align_poses, loop_constraint).  The photometric equation (map_photo.hip) linearises
// the image over +-1 pixel, so it pulls the right way only within about a quarter of the finest texture wavelength;
// halving the frame doubles that distance in metres.  Nothing in the sums or the step kernels changes: a level is a
// smaller frame with its own intrinsics, given to the entry points that exist.
//
// The rule.  Level 0 is the frame.  Level l + 1 has W' = W / 2, H' = H / 2 (integer division: an odd last column or row
// is dropped).  The coarse pixel (i, j) is made from a, b, c, e = X[2j, 2i], X[2j, 2i+1], X[2j+1, 2i], X[2j+1, 2i+1], in
// float32 with one rounding per operation in the order written, no contraction, correctly rounded division, comparisons
// false for a NaN:
//   depth      valid = each of the four > 0 and < inf, and max * keep <= min (keep = 1 - rho_p, one float32 value taken
//              on the host: the block does not straddle a depth step);
//              inv = ((1/a + 1/b) + (1/c + 1/e)) * 0.25f;   d' = 1 / inv where valid, otherwise 0.
//              Inverse depth is affine in the pixel coordinates on a plane (map_refine.hip): the mean of the four is the
//              plane's inverse depth at the block's centre, exact up to rounding.
//   intensity  Y' = ((a + b) + (c + e)) * 0.25f, unconditionally: a NaN or a value outside 0 .. 1 survives and the
//              photometric rule (info_in01) rejects it at the row.
//   intrinsics pixel u lies at the integer u (map_dev.h), the centre of a block at 2i + 0.5; on the host, in float32:
//              fx' = fx * 0.5f, fy' = fy * 0.5f, cx' = (cx - 0.5f) * 0.5f, cy' = (cy - 0.5f) * 0.5f.
// Every level is made from the previous level's rounded float32 values: the result is the rule applied level by level,
// and tests/map_pyramid_ref.py does exactly that in numpy.
//
// k_map_pyramid, one launch for all levels of both images.  A workgroup of 256 threads takes a 32 x 32 tile of level 0;
// thread t owns the level-1 pixel (t % 16, t / 16) of the tile and reads its 2 x 2 block of each image as two 8-byte
// loads: the 16 lanes of a tile row read 128 contiguous bytes, a wave four such rows per instruction.  The level-1 pixel
// goes to global memory and to LDS; the first 64, 16 and 4 threads make levels 2, 3 and 4 from LDS between barriers
// (the compiler reads a block's two rows with one ds_read2_b64.  At level 2 a block row is 32 dwords from the next, the
// bank modulus of that instruction, so the eight lanes of a column share their banks: an 8-way conflict on two reads per
// image and tile, tens of cycles beside a launch of microseconds -- an odd row pitch would cure it and cost the 8-byte
// alignment of the reads; not done).  Every level-0 pixel is read once, every output pixel is written once with a plain
// vector store; no atomics, no scratch, nothing zeroed in front.
// A thread whose pixel lies outside W' x H' of its level writes nothing to global memory and 0 to LDS; a pixel of level
// l + 1 exists only where its four parents exist (integer division guarantees it), so such a 0 is never used for a
// pixel that is written.  A level-0 row of odd width starts on a 4-byte boundary only: the 8-byte loads are declared
// with 4-byte alignment, which global_load_dwordx2 takes.
#include "gsloc_internal.h"
#include "map_dev.h"

namespace gsl {

constexpr int PYR_THREADS = 256;
constexpr int PYR_TILE = 32;  // level-0 pixels per tile side; 32 >> GSL_MAP_PYRAMID_MAX_LEVELS = 2
constexpr int PYR_SIDE = PYR_TILE / 2;  // level-1 pixels per tile side: one per thread
static_assert(GSL_MAP_PYRAMID_MAX_LEVELS == 4 && PYR_SIDE * PYR_SIDE == PYR_THREADS,
              "k_map_pyramid makes levels 2 .. 4 from LDS by 64, 16 and 4 threads");

struct PyrLevels {  // per level 1 .. 4 (index l - 1): its size and where it starts in the packed output, in floats
  int w[GSL_MAP_PYRAMID_MAX_LEVELS], h[GSL_MAP_PYRAMID_MAX_LEVELS];
  long long at[GSL_MAP_PYRAMID_MAX_LEVELS];
};

struct __attribute__((packed, aligned(4))) PyrPair {  // two neighbours of a row, 4-byte aligned: one dwordx2
  float lo, hi;
};

__device__ static inline float pyr_depth(float a, float b, float c, float e, float keep) {
#pragma clang fp contract(off)
  const bool finite = a > 0.f && a < INFINITY && b > 0.f && b < INFINITY && c > 0.f && c < INFINITY && e > 0.f &&
                      e < INFINITY;
  const float hi = fmaxf(fmaxf(a, b), fmaxf(c, e)), lo = fminf(fminf(a, b), fminf(c, e));
  const float inv = ((1.f / a + 1.f / b) + (1.f / c + 1.f / e)) * 0.25f;
  return finite && hi * keep <= lo ? 1.f / inv : 0.f;
}

__device__ static inline float pyr_mean(float a, float b, float c, float e) {
#pragma clang fp contract(off)
  return ((a + b) + (c + e)) * 0.25f;
}

template <bool PHOTO>
__global__ __launch_bounds__(PYR_THREADS) void k_map_pyramid(const float* __restrict__ depth,
                                                             const float* __restrict__ intensity, int width, int levels,
                                                             float keep, PyrLevels lv, float* __restrict__ depth_out,
                                                             float* __restrict__ intensity_out) {
#pragma clang fp contract(off)
  // level l of the tile is (32 >> l)^2 floats: level 1 at 0, level 2 at 256, level 3 at 320 (level 4 is not kept)
  __shared__ float sd[256 + 64 + 16];
  __shared__ float sy[PHOTO ? 256 + 64 + 16 : 1];
  const int t = threadIdx.x;
  {
    const int lx = t & 15, ly = t >> 4;
    const int i = blockIdx.x * 16 + lx, j = blockIdx.y * 16 + ly;
    float d = 0.f, y = 0.f;
    if (i < lv.w[0] && j < lv.h[0]) {  // then rows 2j, 2j + 1 and columns 2i, 2i + 1 are inside level 0
      const size_t top = (size_t)(2 * j) * width + 2 * i, out = (size_t)j * lv.w[0] + i;
      const PyrPair r0 = *(const PyrPair*)(depth + top), r1 = *(const PyrPair*)(depth + top + width);
      d = pyr_depth(r0.lo, r0.hi, r1.lo, r1.hi, keep);
      depth_out[lv.at[0] + out] = d;
      if (PHOTO) {
        const PyrPair y0 = *(const PyrPair*)(intensity + top), y1 = *(const PyrPair*)(intensity + top + width);
        y = pyr_mean(y0.lo, y0.hi, y1.lo, y1.hi);
        intensity_out[lv.at[0] + out] = y;
      }
    }
    sd[t] = d;
    if (PHOTO) sy[t] = y;
  }
  int from = 0, side = 16;  // the previous level's offset in LDS and its tile side
#pragma unroll
  for (int l = 1; l < GSL_MAP_PYRAMID_MAX_LEVELS; ++l) {
    if (l >= levels) return;  // uniform over the workgroup
    __syncthreads();
    const int half = side >> 1, to = from + side * side;
    if (t < half * half) {
      const int lx = t % half, ly = t / half;
      const int i = blockIdx.x * half + lx, j = blockIdx.y * half + ly;
      const int p = from + (2 * ly) * side + 2 * lx;
      const bool exists = i < lv.w[l] && j < lv.h[l];
      const size_t out = (size_t)lv.at[l] + (size_t)j * lv.w[l] + i;
      const float d = pyr_depth(sd[p], sd[p + 1], sd[p + side], sd[p + side + 1], keep);
      if (exists) depth_out[out] = d;
      if (l + 1 < GSL_MAP_PYRAMID_MAX_LEVELS) sd[to + t] = exists ? d : 0.f;
      if (PHOTO) {
        const float y = pyr_mean(sy[p], sy[p + 1], sy[p + side], sy[p + side + 1]);
        if (exists) intensity_out[out] = y;
        if (l + 1 < GSL_MAP_PYRAMID_MAX_LEVELS) sy[to + t] = y;
      }
    }
    from = to;
    side = half;
  }
}

static bool pyramid_shape_ok(int width, int height, int levels) {
  return map_image_ok(width, height) && levels >= 1 && levels <= GSL_MAP_PYRAMID_MAX_LEVELS &&
         (width >> levels) >= 4 && (height >> levels) >= 4;
}

}  // namespace gsl

extern "C" int64_t gsl_map_pyramid_floats(int width, int height, int levels) {
  if (!gsl::pyramid_shape_ok(width, height, levels)) return 0;
  int64_t n = 0;
  for (int l = 1; l <= levels; ++l) n += (int64_t)(width >> l) * (height >> l);
  return n;
}

extern "C" int gsl_map_pyramid(const float* depth, const float* intensity, int width, int height, int levels, float keep,
                               float* depth_out, float* intensity_out, void* stream) {
  if (!depth || !depth_out || (intensity == nullptr) != (intensity_out == nullptr)) return GSL_ERR_BAD_ARG;
  if (!gsl::pyramid_shape_ok(width, height, levels) || !(keep > 0.f && keep <= 1.f)) return GSL_ERR_BAD_ARG;
  gsl::PyrLevels lv = {};
  long long at = 0;
  for (int l = 1; l <= levels; ++l) {
    lv.w[l - 1] = width >> l;
    lv.h[l - 1] = height >> l;
    lv.at[l - 1] = at;
    at += (long long)lv.w[l - 1] * lv.h[l - 1];
  }
  const dim3 grid((unsigned)((lv.w[0] + 15) / 16), (unsigned)((lv.h[0] + 15) / 16));
  if (intensity)
    hipLaunchKernelGGL(gsl::k_map_pyramid<true>, grid, dim3(gsl::PYR_THREADS), 0, (hipStream_t)stream, depth, intensity,
                       width, levels, keep, lv, depth_out, intensity_out);
  else
    hipLaunchKernelGGL(gsl::k_map_pyramid<false>, grid, dim3(gsl::PYR_THREADS), 0, (hipStream_t)stream, depth, intensity,
                       width, levels, keep, lv, depth_out, intensity_out);
  GSL_CHECK_LAUNCH();
  return GSL_OK;
}
