// What crosses translation units inside libgsloc_hip and is not part of the C ABI (include/gsloc_hip.h): every function
// one .hip file defines and another calls is declared here, once; plus the host-side argument checks and the
// (channels, ed) -> template dispatch that the entry points share.  The functions are C++ (namespace gsl), not C symbols.
#pragma once
#include "gsloc_common.h"

namespace gsl {

struct LongWs;     // long_dev.h
struct InfoPhoto;  // map_info_dev.h

// misc.hip: zero n dwords with a kernel of the library (never hipMemsetAsync: see the note there)
int zero_u32(void* p, size_t n_dwords, hipStream_t st);

// compact.hip: launch of k_count_scan, the single-workgroup exclusive scan of nb workgroup counts -> bases[nb],
// total -> total[0] (any nb: a thread owns a contiguous chunk), between the two passes of an ordered compaction
// (compact_dev.h); the caller checks the launch
void launch_count_scan(hipStream_t st, const uint32_t* counts, int nb, uint32_t* bases, int32_t* total);

// binning.hip: the launches of two-pass binning that the staged API and the fused pipeline share (the caller checks the
// launch).  The scan of the tile counts -> tile_offsets[n_tiles + 1], total, cursors zeroed, counts cleared; and the
// scatter of the (depth bits, id) keys of the Q0 records into the tile buckets (order_ids: NULL, or the id of every slot)
void launch_tile_scan(hipStream_t st, int32_t* counts, int n_tiles, int32_t* tile_offsets, int32_t* n_isects,
                      int32_t* cursors);
void launch_record_scatter(hipStream_t st, const float* Q0, const int32_t* radii, const int32_t* order_ids, int N,
                           int tile_w, int tile_h, int ty0, int ty1, const int32_t* tile_offsets, int32_t* cursors,
                           long long capacity, uint64_t* keys);

// tile_sort.hip: gsl_tile_sort that can also leave the sorted (depth bits, id) keys in sort_keys and read the unsorted keys
// from fixed-capacity per-tile bins instead of sort_keys (gsl_fused_bin), and zero clear_n 64-byte gradient rows at
// clear_rows along the way (gsl_fused_bin_clear; NULL / 0: none) -- with a launch of their own where no sort launches
int tile_sort_keys(int32_t* tile_offsets, int tile_begin, int n_strip_tiles, int64_t capacity, uint64_t* sort_keys,
                   int32_t* flatten_ids, int64_t* isect_ids, int64_t cam_enc, int write_sorted_keys, uint64_t* bins,
                   int bin_cap, const int32_t* counts, int32_t* n_isects, int32_t* flags, int long_min, int occupied_tiles,
                   const int32_t* storage_of, float* clear_rows, int clear_n, void* stream);

// raster_px.hip: launch of k_long_map (one workgroup lists the (tile, segment) pairs of the strip's long tiles in w);
// the caller checks the launch
void launch_long_map(hipStream_t st, const int32_t* tile_offsets, int tile_begin, int n_strip_tiles, long long capacity,
                     int long_min, int max_seg, int max_list, const LongWs& w);

// raster_det.hip: launch of the deterministic compositing backward k_mraster_bwd (arguments as checked by
// gsl_fused_raster_bwd, raster_g16.hip); vrow gets one gradient row per intersection
int launch_mraster_bwd(const float* Q0, const float* Q1, const float* Q2, int channels, int ed, int width, int height,
                       int tile_w, int ty0, int ty1, const int32_t* tile_offsets, const int32_t* flatten_ids,
                       int64_t capacity, const float* render, const float* alphas, const int32_t* last_ids,
                       const float* v_render, const float* v_alphas, float* vrow, int row0, int row1, const void* Qh,
                       hipStream_t st);

// map_info.hip: the zeroing of out[GSL_MAP_INFO_VALUES] and the launch of k_map_pose_info, for arguments checked as
// gsl_map_pose_info checks them; w2c on the device.  Returns GSL_OK or the status of the failed launch
int map_pose_info_launch(const float* means, int64_t n_rows, const float* w2c, float fx, float fy, float cx, float cy,
                         const float* depth, int width, int height, float keep, float beyond, float kappa,
                         float near_plane, int64_t* out, hipStream_t st);

// map_photo.hip: the same with k_map_pose_info_photo, for arguments checked as gsl_map_pose_info_photo checks them;
// extra NULL or the two words, which are then zeroed as well
int map_pose_info_photo_launch(const float* means, int64_t n_rows, const float* w2c, float fx, float fy, float cx,
                               float cy, const float* depth, int width, int height, float keep, float beyond,
                               float kappa, float near_plane, int64_t* out, const InfoPhoto& photo, int64_t* extra,
                               hipStream_t st);

// ---- workspace of the fused pipeline (sized by gsl_fused_ws_bytes, fused_project.hip) -------------------------------
// ws = [tile_counts n_tiles][cursors n_tiles][pad to 16 bytes][pose-gradient rows ceil(N/256) x 16 floats][stage rows]
#define GSL_VM_STAGE_ROWS 64  // scratch rows behind the ceil(N / 256) pose-gradient rows: stage 1 of the row reduction
static inline size_t fused_vm_rows_offset(int n_tiles) { return ((size_t)2 * (size_t)n_tiles * sizeof(int32_t) + 15) & ~(size_t)15; }
// state word of the binned mode's counter contract: the 16th float of the first pose-gradient row (rows use 15)
static inline int32_t* fused_bin_state(void* ws, int n_tiles) {
  return (ws && n_tiles > 0) ? (int32_t*)((char*)ws + fused_vm_rows_offset(n_tiles)) + 15 : nullptr;
}

// ---- shared by the compositing entry points -------------------------------------------------------------------------
// Frame geometry, checked first: a positive frame and tile grid, the tile strip [ty0, ty1) inside the grid, pixel rows
// [row0, row1) in order, no negative capacity, and (cover; the long-list entry points have never asked for it) 16-pixel
// tiles that cover the frame.
static inline bool frame_ok(int width, int height, int tile_w, int tile_h, int ty0, int ty1, int64_t capacity, int row0,
                            int row1, bool cover = true) {
  if (width <= 0 || height <= 0 || tile_w <= 0 || tile_h <= 0 || ty0 < 0 || ty1 > tile_h || ty0 > ty1 || capacity < 0 ||
      row0 < 0 || row0 > row1)
    return false;
  return !cover || (tile_w * 16 >= width && tile_h * 16 >= height);
}
// The records of this channel count are there (the fp16-staged array Qh, or Q0 / Q1 and Q2 where there are colours), and
// no expected depth without a depth channel.  Two calls, because the entry points place them on either side of their
// early "nothing to do" returns, and the status of every bad argument is pinned (tests/test_entry_checks_cpu.py).
static inline bool records_ok(const void* Qh, const float* Q0, const float* Q1, const float* Q2, int channels) {
  return Qh || (Q0 && Q1 && (channels < 3 || Q2));
}
static inline bool ed_ok(int channels, int ed) { return !(ed && channels == 3); }

}  // namespace gsl

// CALL(D, ED) with the template arguments of a (channels, ed) pair of the fused pipeline: depth, RGB, RGB + depth; ED
// (expected depth) only where there is a depth channel.  Any other channel count leaves the function with GSL_ERR_BAD_ARG.
#define GSL_DISPATCH_CH_ED(D, ED, CALL)                            \
  if (D == 1) { if (ED) CALL(1, true); else CALL(1, false); }      \
  else if (D == 3) { CALL(3, false); }                             \
  else if (D == 4) { if (ED) CALL(4, true); else CALL(4, false); } \
  else return GSL_ERR_BAD_ARG;
