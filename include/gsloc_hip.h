/*
 * gsloc_hip.h -- C ABI of libgsloc_hip.so: the MI355X (gfx950) Gaussian-splat
 * rasterizer behind GsplatLoc's pose-tracking loop.
 *
 * Boundary being replaced.  The reference reaches this arithmetic through the
 * third-party pybind11/torch extension `gsplat.csrc` (`_C`, IDX:14216 of
 * /root/reference/.vscode/PythonImportHelper-v2-Completion.json) whose Python
 * wrappers are called from /root/reference/src/my_gsplat/model.py:195-213 and
 * /root/reference/src/my_gsplat/geometry.py:117-132.  Nothing C-callable exists
 * in the reference; every entry point below names the gsplat operator (IDX line)
 * whose work it performs, and INTEGRATION.md shows the ctypes binding.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer unless the name ends in `_host`;
 *   - all floating point data is fp32, row-major, contiguous; indices are int32,
 *     intersection keys int64;
 *   - `stream` is a hipStream_t passed as void* (0 = default stream);
 *   - no allocation, no host synchronisation, no global state inside any call
 *     (safe to capture in a hipGraph; the one exception is the host-side launch
 *     counter behind gsl_dev_tile_sort_launches); scratch comes from the caller through the
 *     `*_ws` arguments, sized by the matching `*_ws_bytes` query;
 *   - return value: GSL_OK (0) or a negative gsl_status; the launch error of the
 *     last kernel (hipGetLastError) is reported as GSL_ERR_HIP.
 */
#ifndef GSLOC_HIP_H
#define GSLOC_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum gsl_status {
  GSL_OK = 0,
  GSL_ERR_BAD_ARG = -1,   /* null pointer / non-positive size / unsupported channel count */
  GSL_ERR_WORKSPACE = -2, /* workspace too small */
  GSL_ERR_HIP = -3        /* HIP runtime reported an error for a launch */
} gsl_status;

/* Library identification: returns "gsloc_hip <version> gfx950". */
const char* gsl_version(void);
/* Text for a gsl_status. */
const char* gsl_status_string(int status);
/* Diagnostics (tests): fill the LDS of every CU with `pattern` (e.g. 0xFFFFFFFF, a NaN), to show that no kernel of the
 * library reads LDS it has not written. */
int gsl_dev_poison_lds(uint32_t pattern, void* stream);
/* Diagnostics (tests): how many launches of one tile-sort kernel this process has issued (host-side counters, no
 * device work; a launch recorded into a captured graph counts once, at capture).  variant 0 = k_tile_sort<4> (16 keys
 * per lane), 1 = k_tile_sort<5> (32 keys per lane), 2 = k_tile_sort_wg; -1 for any other variant. */
int64_t gsl_dev_tile_sort_launches(int variant);
/* ---- projection: gsplat.fully_fused_projection fwd/bwd (IDX:14351, IDX:14270) ----
 * One camera.  viewmat[16] world->camera row-major, K[9] intrinsics, both on device.
 * Outputs for culled Gaussians: radii = 0, other outputs 0.
 * compensations may be NULL (rasterize_mode "classic"). */
int gsl_project_fwd(const float* means, const float* quats, const float* scales,
                    const float* viewmat, const float* K, int N, int width, int height,
                    float eps2d, float near_plane, float far_plane, float radius_clip,
                    int32_t* radii, float* means2d, float* depths, float* conics,
                    float* compensations, void* stream);

/* vjp of the above.  v_means/v_quats/v_scales may be NULL together (pose-only
 * mode); v_viewmat may be NULL.  v_viewmat[16] is OVERWRITTEN with this camera's
 * gradient (rows 0..2 used; row 3 zero).  v_compensations may be NULL.
 * ws: gsl_project_bwd_ws_bytes(N) bytes. */
size_t gsl_project_bwd_ws_bytes(int N);
int gsl_project_bwd(const float* means, const float* quats, const float* scales,
                    const float* viewmat, const float* K, int N, int width, int height,
                    float eps2d, const int32_t* radii, const float* conics,
                    const float* compensations, const float* v_means2d, const float* v_depths,
                    const float* v_conics, const float* v_compensations, float* v_means,
                    float* v_quats, float* v_scales, float* v_viewmat, void* ws, size_t ws_bytes,
                    void* stream);

/* ---- packed projection: gsplat.fully_fused_projection(packed=True) fwd/bwd ----
 * All C cameras in one call: viewmats[C,16], Ks[C,9].  Of the C*N (camera, Gaussian) pairs, those gsl_project_fwd
 * gives radii > 0 get one output row each, in ascending order of camera * N + gaussian (camera c's rows are one
 * contiguous slice); a row holds the bits gsl_project_fwd writes for that pair.  C * N must be below 2^31.
 *
 * gsl_project_packed_count: evaluates the cull, leaves one ballot per wave and the row offset of every workgroup in
 *   ws (gsl_project_packed_ws_bytes(C, N)) and writes the number of rows to nnz[1].  The caller reads nnz back to
 *   size the outputs (the one host round trip of packed mode, as in gsplat).
 * gsl_project_packed_fill: after gsl_project_packed_count with the same arguments and the same, untouched ws.
 *   Writes camera_ids[nnz], gaussian_ids[nnz] (int64, as gsplat), radii[nnz], means2d[nnz,2], depths[nnz],
 *   conics[nnz,3] and, if not NULL, compensations[nnz].  Rows at positions >= capacity are dropped. */
size_t gsl_project_packed_ws_bytes(int C, int N);
int gsl_project_packed_count(const float* means, const float* quats, const float* scales,
                             const float* viewmats, const float* Ks, int C, int N, int width,
                             int height, float eps2d, float near_plane, float far_plane,
                             float radius_clip, int32_t* nnz, void* ws, size_t ws_bytes, void* stream);
int gsl_project_packed_fill(const float* means, const float* quats, const float* scales,
                            const float* viewmats, const float* Ks, int C, int N, int width,
                            int height, float eps2d, float near_plane, float far_plane,
                            float radius_clip, int64_t capacity, int64_t* camera_ids,
                            int64_t* gaussian_ids, int32_t* radii, float* means2d, float* depths,
                            float* conics, float* compensations, void* ws, size_t ws_bytes,
                            void* stream);

/* vjp of the above, one thread per packed row; camera_ids must be ascending (as the fill pass writes them), rows
 * whose ids lie outside [0,C) x [0,N) are skipped.  v_means/v_quats/v_scales may be NULL together, v_viewmats may be
 * NULL, v_compensations may be NULL.
 *   sparse == 0: v_means[N,3], v_quats[N,4], v_scales[N,3] are OVERWRITTEN with the sum over the cameras (zero for a
 *     Gaussian without a row; plain stores for C == 1, float atomics -- summation order not fixed -- for C > 1);
 *   sparse != 0: they are the value rows [nnz,3], [nnz,4], [nnz,3] of a sparse gradient indexed by gaussian_ids.
 * v_viewmats[C,16] is OVERWRITTEN (rows 0..2 used, row 3 zero; fixed summation order).
 * ws: gsl_project_packed_bwd_ws_bytes(nnz, C), needed when v_viewmats is given. */
size_t gsl_project_packed_bwd_ws_bytes(int64_t nnz, int C);
int gsl_project_packed_bwd(const float* means, const float* quats, const float* scales,
                           const float* viewmats, const float* Ks, int C, int N, int width, int height,
                           float eps2d, int64_t nnz, const int64_t* camera_ids,
                           const int64_t* gaussian_ids, const float* conics,
                           const float* compensations, const float* v_means2d, const float* v_depths,
                           const float* v_conics, const float* v_compensations, int sparse,
                           float* v_means, float* v_quats, float* v_scales, float* v_viewmats, void* ws,
                           size_t ws_bytes, void* stream);

/* Rows of a per-Gaussian (or per-camera) array for the packed rows, and the vjp: what x[gaussian_ids] and its
 * backward are in gsplat's packed rasterization.  D floats per row, ids int64.
 * gsl_gather_rows: dst[nnz,D], dst[r] = src[ids[r]] (a zero row for an id outside [0, n_src)).
 * gsl_scatter_add_rows: v_dst[n_dst,D] is OVERWRITTEN with the sum of the v_rows[nnz,D] that name each row (rows
 *   nobody names are zero).  unique != 0: the caller guarantees that no id occurs twice (plain stores); otherwise
 *   float atomics (summation order not fixed), one per wave where all its lanes hold the same id.
 *   nnz, n_dst < 2^31. */
int gsl_gather_rows(const float* src, int64_t n_src, int D, const int64_t* ids, int64_t nnz,
                    float* dst, void* stream);
int gsl_scatter_add_rows(const float* v_rows, const int64_t* ids, int64_t nnz, int D, int64_t n_dst,
                         int unique, float* v_dst, void* stream);

/* ---- map growth: the pixels of a depth frame that the map does not explain are appended to it ----
 * Images are [height,width] float32 on the device, row-major: depth (observed, metres), render_depth and alphas (the
 * map's expected-depth render and its alpha at the frame's pose); rgb[height,width,3] in 0..255.  width * height must
 * be below 2^31.
 *
 * A pixel is selected when depth is finite and > 0 and (alphas < alpha_min or depth < render_depth * keep), evaluated
 * in float32 exactly as written (one rounded product).  render_depth == NULL and alphas == NULL together ("no render
 * yet"): every pixel with a finite depth > 0 is selected.
 *
 * gsl_map_select: evaluates the rule, leaves one ballot per wave and the row offset of every workgroup in ws
 *   (gsl_map_ws_bytes(width, height)), writes the number of selected pixels to n_new[0] and 0 to n_new[1].
 * gsl_map_append: after gsl_map_select with the same depth, size and the same, untouched ws.  The selected pixels
 *   (u, v), in raster order, become rows n_live, n_live + 1, ... of means[capacity,3] and colors[capacity,3]:
 *   mean = R p + t with p = ((u - cx) / fx * depth, (v - cy) / fy * depth, depth) and [R | t] the rows of c2w[16]
 *   (camera-to-world, row-major, on the device), colour = rgb / 255; float32, no fused operations.  Rows at or beyond
 *   capacity are dropped -- nothing is written there -- and the number of rows written goes to n_new[1].
 * Both return GSL_ERR_BAD_ARG before any launch for a NULL array, a non-positive size, n_live outside [0, capacity],
 * only one of render_depth / alphas, or a workspace smaller than gsl_map_ws_bytes. */
size_t gsl_map_ws_bytes(int width, int height);
int gsl_map_select(const float* render_depth, const float* alphas, const float* depth, int width,
                   int height, float alpha_min, float keep, int32_t* n_new, void* ws, size_t ws_bytes,
                   void* stream);
int gsl_map_append(const float* depth, const float* rgb, int width, int height, float fx, float fy,
                   float cx, float cy, const float* c2w, float* means, float* colors, int64_t n_live,
                   int64_t capacity, int32_t* n_new, void* ws, size_t ws_bytes, void* stream);

/* ---- local map: the rows of the map that are in view from a pose, compacted in map order (csrc/map_view.hip) ----
 * Row i of means[n_rows,3] is IN VIEW when, with w2c[16] (world to camera, row-major, on the device),
 *   x = ((w0 px + w1 py) + w2 pz) + w3, and y, z likewise from rows 1 and 2 of w2c;  z > near_plane and z < far_plane;
 *   u = fx x / z + cx and v = fy y / z + cy satisfy -guard_px <= u <= (width - 1) + guard_px and
 *   -guard_px <= v <= (height - 1) + guard_px;
 * float32, evaluated exactly as written (no fused operation, correctly rounded division, the two upper limits one
 * rounded sum each), comparisons false for a NaN.  counters is int32[3].  n_rows must be below 2^31.
 *
 * gsl_map_view_select: evaluates the rule, leaves one ballot per wave and the row offset of every workgroup in ws
 *   (gsl_map_view_ws_bytes(n_rows)); counters[0] = rows in view, counters[1] = rows in view whose bit is CLEAR in the
 *   ballots of prev_ws -- a workspace an earlier call filled for the same n_rows, only read, not ws -- or 0 when
 *   prev_ws is NULL; counters[2] = 0.
 * gsl_map_view_gather: after gsl_map_view_select on the same rows and the same, untouched ws.  The selected rows, in
 *   ascending row index, become rows 0, 1, ... of out_means / out_colors (bit copies of means / colors [n_rows,3]);
 *   their indices go to out_ids (may be NULL).  Rows at or beyond out_capacity are dropped -- nothing is written
 *   there -- and the number of rows written goes to counters[2].
 * Both return GSL_ERR_BAD_ARG before any launch for a NULL array, n_rows <= 0 or >= 2^31, a non-positive image size,
 * fx or fy not non-zero, guard_px negative or NaN, near_plane >= far_plane, prev_ws == ws, out_capacity < 0; and
 * GSL_ERR_WORKSPACE for a workspace smaller than gsl_map_view_ws_bytes. */
size_t gsl_map_view_ws_bytes(int64_t n_rows);
int gsl_map_view_select(const float* means, int64_t n_rows, const float* w2c, float fx, float fy, float cx,
                        float cy, int width, int height, float guard_px, float near_plane, float far_plane,
                        const void* prev_ws, int32_t* counters, void* ws, size_t ws_bytes, void* stream);
int gsl_map_view_gather(const float* means, const float* colors, int64_t n_rows, float* out_means,
                        float* out_colors, int32_t* out_ids, int64_t out_capacity, int32_t* counters, void* ws,
                        size_t ws_bytes, void* stream);

/* ---- local map, occlusion culling: the rows in view that no nearer surface of the map hides (csrc/map_occl.hip) ----
 * The rule of gsl_map_view_select (IN THE BAND below) and a z-buffer of the map's own rows on a coarse grid:
 *   gi = (int)ceilf(guard_px);  cell_px is 1, 2, 4, 8 or 16;  CW = (width - 1 + 2 gi) / cell_px + 1 and
 *   CH = (height - 1 + 2 gi) / cell_px + 1 (integer division);  a row in the band lies in the cell
 *   cu = (int)floorf((u + (float)gi) * (1 / cell_px)), cv = (int)floorf((v + (float)gi) * (1 / cell_px)), which is
 *   inside the grid.  The widened image, width - 1 + 2 gi and height - 1 + 2 gi, must stay below 2^24 pixels a side
 *   and CW * CH at or below 2^26.
 * gsl_map_occl_zbuf_bytes: 4 CW CH, or 0 for arguments the entry points refuse.
 * gsl_map_occl_depth: zbuf[CH,CW] uint32 = 0 where no row in the band falls into the cell, else the maximum of
 *   ~bits(z) over those rows: the complement of the bit pattern of the NEAREST depth (near_plane >= 0, so z > 0 and
 *   its bits order as the float does).  Integer atomics: the same buffer in every run and for every order of the rows.
 * gsl_map_occl_select: with m the minimum of zbuf over the cells (cu + du, cv + dv), |du|, |dv| <= window, a cell
 *   outside the grid counting as 0, a row in the band is OCCLUDED when m != 0 and rho_keep * z > asfloat(~m) (one
 *   rounded product; rho_keep is 1 - rho, the float32 difference taken by the caller), and SELECTED when it is in the
 *   band and not occluded.  Leaves in ws (gsl_map_occl_ws_bytes(n_rows): the layout of gsl_map_view_select, which it
 *   is at least as large as, and two more columns) one ballot per wave of the selected rows and the row offset of every
 *   workgroup, so that gsl_map_view_gather on the same rows and the same, untouched ws moves them.  counters is
 *   int32[4]: [0] rows selected, [1] rows selected whose bit is CLEAR in the ballots of prev_ws (as
 *   gsl_map_view_select; 0 when prev_ws is NULL), [2] = 0 (the gather's), [3] rows in the band and occluded.  zbuf is
 *   only read; it is what gsl_map_occl_depth left for the same image, guard_px and cell_px.
 * float32, evaluated exactly as written, comparisons false for a NaN.  Both return GSL_ERR_BAD_ARG before any launch
 * for a NULL array, n_rows <= 0 or >= 2^31, width or height <= 0 or width * height > 2^31 - 1, fx or fy not non-zero,
 * guard_px negative or NaN, near_plane negative or NaN or >= far_plane, a cell_px other than the five, a grid beyond
 * the limits above, window outside 0..3, rho_keep outside (0, 1), prev_ws == ws; and GSL_ERR_WORKSPACE for a zbuf
 * smaller than gsl_map_occl_zbuf_bytes or a workspace smaller than gsl_map_occl_ws_bytes. */
size_t gsl_map_occl_zbuf_bytes(int width, int height, float guard_px, int cell_px);
size_t gsl_map_occl_ws_bytes(int64_t n_rows);
int gsl_map_occl_depth(const float* means, int64_t n_rows, const float* w2c, float fx, float fy, float cx, float cy,
                       int width, int height, float guard_px, int cell_px, float near_plane, float far_plane,
                       void* zbuf, size_t zbuf_bytes, void* stream);
int gsl_map_occl_select(const float* means, int64_t n_rows, const float* w2c, float fx, float fy, float cx, float cy,
                        int width, int height, float guard_px, float near_plane, float far_plane, int cell_px,
                        int window, float rho_keep, const void* zbuf, size_t zbuf_bytes, const void* prev_ws,
                        int32_t* counters, void* ws, size_t ws_bytes, void* stream);

/* ---- free space: the rows of the map that a depth frame sees through are removed (csrc/map_free.hip) ----
 * depth[height,width] float32 on the device, row-major: the observed depth, metres.  Row i of means[n_rows,3], with
 * w2c[16] (world to camera, row-major, on the device):
 *   x = ((w0 px + w1 py) + w2 pz) + w3, and y, z likewise from rows 1 and 2 of w2c;
 *   u = fx x / z + cx, v = fy y / z + cy;  uf = rintf(u), vf = rintf(v) (round half to even);
 *   TESTED  when z > near_plane and 0 <= uf <= width - 1 and 0 <= vf <= height - 1 (float comparisons, then the
 *           conversion to int; uf = -0 passes and is column 0);
 *   BLOCKED when some pixel (uf + du, vf + dv), |du|, |dv| <= window_px, that lies inside the image has a depth d
 *           that is not (finite and > 0), or not (z < d * keep); pixels of the window outside the image are skipped;
 *   REMOVED when tested and not blocked.
 * float32, evaluated exactly as written (no fused operation, correctly rounded division, d * keep one rounded
 * product), comparisons false for a NaN: NaN / inf rows, rows behind near_plane and rows outside the image are kept,
 * and so is a row with a pixel without depth in its window.  keep is 1 - rho, the float32 difference taken by the
 * caller.  counters is int32[3].
 *
 * gsl_map_free_select: evaluates the rule and leaves, in ws (gsl_map_view_ws_bytes(n_rows), the layout of
 *   gsl_map_view_select), one ballot per wave of the rows that STAY and the row offset of every workgroup;
 *   counters[0] = rows that stay, counters[1] = counters[2] = 0.  gsl_map_view_gather on the same rows and the same,
 *   untouched ws then moves the survivors, in ascending row index, into another buffer (out_ids: the old row of every
 *   survivor; counters[2]: rows stored).  Not in place: a workgroup would overwrite rows another has not read yet.
 * Returns GSL_ERR_BAD_ARG before any launch for a NULL means, w2c, depth, counters or ws, n_rows <= 0 or >= 2^31,
 * width or height <= 0 or width * height > 2^31 - 1, fx or fy not non-zero, keep outside (0, 1], window_px outside
 * 0..3; and GSL_ERR_WORKSPACE for a workspace smaller than gsl_map_view_ws_bytes. */
int gsl_map_free_select(const float* means, int64_t n_rows, const float* w2c, float fx, float fy, float cx, float cy,
                        const float* depth, int width, int height, float keep, int window_px, float near_plane,
                        int32_t* counters, void* ws, size_t ws_bytes, void* stream);

/* ---- bounded map: a last-observed stamp per row, the least recently observed rows evicted (csrc/map_evict.hip) ----
 * stamps[n_rows] int32 on the device: the index of the last frame that observed the row.
 *
 * gsl_map_observe: row i of means[n_rows,3], with w2c[16] (world to camera, row-major, on the device) and
 *   depth[height,width] float32 (the observed depth, metres):
 *   x = ((w0 px + w1 py) + w2 pz) + w3, and y, z likewise from rows 1 and 2 of w2c;
 *   u = fx x / z + cx, v = fy y / z + cy;  uf = rintf(u), vf = rintf(v) (round half to even);
 *   IN REACH when z > near_plane and z < far_plane and -reach_px <= u <= (width - 1) + reach_px and
 *            -reach_px <= v <= (height - 1) + reach_px (the rule of gsl_map_view_select with guard_px = reach_px);
 *   INSIDE   when 0 <= uf <= width - 1 and 0 <= vf <= height - 1 (float comparisons; uf = -0 is column 0);
 *   AGREES   when some pixel (uf + du, vf + dv), |du|, |dv| <= window_px, that lies inside the image has a depth d
 *            that is finite and > 0 with z >= d * keep and z * keep <= d (two rounded products, no division);
 *   OBSERVED when in reach and (not inside, or agrees): a row in the band around the image paints into the frame and
 *            there is no depth to hold it against.
 *   Observed rows get stamps[i] = now, every other row keeps its stamp.  float32, evaluated exactly as written (no
 *   fused operation, correctly rounded division, the two upper limits one rounded sum each), comparisons false for a
 *   NaN: NaN / inf rows are never observed.  keep is 1 - rho, the float32 difference taken by the caller.
 *
 * gsl_map_evict_select: integers only.  age = clamp(now - stamp, 0, 1023) (the difference taken in 64 bits); a row is
 *   EVICTABLE when age >= min_age; E = min(need, evictable rows); a* = the largest age with count(age >= a*) >= E.
 *   EVICTED are the rows with age > a* and, of the rows with age == a*, the first E - count(age > a*) (the tie quota)
 *   in ascending row index.  need == 0 or nothing evictable: E = 0, a* = 1023, every row stays.
 *   Leaves in the head of ws -- gsl_map_view_ws_bytes(n_rows) bytes, the layout of gsl_map_view_select -- one ballot
 *   per wave of the rows that STAY and the row offset of every workgroup; counters[0] = rows that stay,
 *   counters[1] = E, counters[2] = 0.  gsl_map_view_gather on the same rows and the same, untouched ws then moves the
 *   survivors into another buffer (out_ids: the old row of every survivor).  Behind the head, with
 *   nb = ceil(n_rows / 256): the ballots of age == a*, nb x 4 uint64; the 1024 age bins, uint32; and uint32
 *   a*, the tie quota, E, count(age == a*).  counters is int32[3].
 * gsl_map_gather_i32: dst[r] = src[ids[r]] for r < n_ids (0 for an id outside [0, n_src)): the stamps follow the rows
 *   that gsl_map_view_gather moved, with the ids it wrote.  n_ids == 0 does nothing.
 *
 * All return GSL_ERR_BAD_ARG before any launch for a NULL array, n_rows (n_src) <= 0 or >= 2^31, n_ids < 0 or >= 2^31,
 * width or height <= 0 or width * height > 2^31 - 1, fx or fy not non-zero, keep outside (0, 1], window_px outside
 * 0..3, reach_px negative or NaN, near_plane >= far_plane, need < 0, min_age < 1; and GSL_ERR_WORKSPACE for a
 * workspace smaller than gsl_map_evict_ws_bytes. */
int gsl_map_observe(const float* means, int64_t n_rows, const float* w2c, float fx, float fy, float cx, float cy,
                    const float* depth, int width, int height, float keep, int window_px, float reach_px,
                    float near_plane, float far_plane, int now, int32_t* stamps, void* stream);
size_t gsl_map_evict_ws_bytes(int64_t n_rows);
int gsl_map_evict_select(const int32_t* stamps, int64_t n_rows, int now, int min_age, int64_t need,
                         int32_t* counters, void* ws, size_t ws_bytes, void* stream);
int gsl_map_gather_i32(const int32_t* src, int64_t n_src, const int32_t* ids, int64_t n_ids, int32_t* dst,
                       void* stream);

/* ---- map resolution: the rows that share a voxel of side h are fused into one (csrc/map_merge.hip) ----
 * means[n_rows,3], colors[n_rows,3] float32 and stamps[n_rows] int32 on the device, as in the map.  h and inv_h are
 * float32 values taken by the caller: h = (float)merge_voxel, inv_h = 1.0f / h (one correctly rounded division).
 * The rule is evaluated exactly as written: float32 with no fused operation where float32 is named, IEEE double
 * elsewhere.
 *   CELL      for each axis a: f_a = p_a * inv_h (one rounded product), c_a = floorf(f_a);
 *   MERGEABLE when the three f_a are finite and |c_a| <= 2^20 - 1.  Every other row -- NaN, inf, too far for a key of
 *             3 x 21 bits -- stays as it is, and no other row is ever merged with it.  The voxel key is the three
 *             cells, each biased by 2^20 - 1, packed into 63 bits (axis a at bit 21 a); the all-ones word is the empty
 *             slot of the table;
 *   VOXEL STATISTICS over the k mergeable rows of a voxel: first = the smallest row index;
 *             S_a = the integer sum of q_a = (uint32)rintf((f_a - c_a) * 65536.f);
 *             C_j = the integer sum of rintf(fminf(fmaxf(colour_j, 0.f), 1.f) * 65280.f) -- 65280 = 255 * 256, so that
 *             8-bit colours are exact; a NaN colour counts as 0;  T = the largest stamp;
 *   k == 1    the row keeps every bit of its mean, colour and stamp;
 *   k > 1     the rows other than first are REMOVED, and row first becomes
 *             mean_a   = (float)(((double)c_a + (double)S_a / (65536.0 * (double)k)) * (double)h),
 *             colour_j = (float)((double)C_j / (65280.0 * (double)k)),  stamp = T;
 *   ORDER     the rows that stay keep their map order.
 * All sums are integers: the result does not depend on the order in which the rows arrive, nor on the table's hash.
 *
 * gsl_map_merge_select: evaluates the rule over the rows and leaves, in the head of ws -- gsl_map_view_ws_bytes(n_rows)
 *   bytes, the layout of gsl_map_view_select -- one ballot per wave of the rows that STAY and the row offset of every
 *   workgroup; behind the head the voxel table (the smallest power of two >= 2 n_rows slots, open addressing), the
 *   voxel sums, the slot of every row, and h.  counters is int32[4]: counters[0] = rows that stay, counters[1] = rows
 *   removed, counters[2] = 0, counters[3] = 0 -- or 1 when some row found no slot within as many probes as the table
 *   has slots (it was then treated as not mergeable; with a table half empty this cannot happen, and a caller that
 *   reads 1 must not trust the result).
 * gsl_map_view_gather on the same rows and the same, untouched ws then moves the survivors into another buffer
 *   (out_ids: the old row of every survivor, counters[2]: rows stored), and gsl_map_gather_i32 their stamps.
 * gsl_map_merge_apply: after those, with the same n_rows and the same, untouched ws; ids = the out_ids of the gather,
 *   out_means / out_colors / out_stamps = what the gathers filled.  For r < counters[2] (read on the device): where the
 *   voxel of old row ids[r] has k > 1, rows r of the three outputs are overwritten by the rule.
 *
 * Both return GSL_ERR_BAD_ARG before any launch for a NULL array, n_rows <= 0 or >= 2^31, h or inv_h not finite and
 * positive; and GSL_ERR_WORKSPACE for a workspace smaller than gsl_map_merge_ws_bytes. */
size_t gsl_map_merge_ws_bytes(int64_t n_rows);
int gsl_map_merge_select(const float* means, const float* colors, const int32_t* stamps, int64_t n_rows, float inv_h,
                         float h, int32_t* counters, void* ws, size_t ws_bytes, void* stream);
int gsl_map_merge_apply(const int32_t* ids, const int32_t* counters, int64_t n_rows, float* out_means,
                        float* out_colors, int32_t* out_stamps, void* ws, size_t ws_bytes, void* stream);

/* ---- pose scores: how many rows of the map a depth frame confirms from each of n_poses poses (csrc/map_score.hip) ----
 * depth[height,width] float32 on the device, row-major: the observed depth, metres.  w2c[n_poses,16]: world to camera,
 * row-major, on the device.  counts[n_poses,3] int32 on the device; it need not be initialised, the entry point zeroes
 * it on the stream.  Row i of means[n_rows,3], pose k, with w the rows of w2c[k]:
 *   x = ((w0 px + w1 py) + w2 pz) + w3, and y, z likewise from rows 1 and 2 of w2c[k];
 *   u = fx x / z + cx, v = fy y / z + cy;  uf = rintf(u), vf = rintf(v) (round half to even);
 *   TESTED when z > near_plane and 0 <= uf <= width - 1 and 0 <= vf <= height - 1 (float comparisons, then the
 *          conversion to int; uf = -0 passes and is column 0) and the row's own pixel d = depth[vf, uf] is finite
 *          and > 0 -- no window;
 *   FRONT  when tested and z < d * keep;  BEHIND when tested and z > d * beyond (one rounded product each);
 *   AGREE  when tested and neither: z == d * keep and z == d * beyond agree;
 *   counts[k] = (rows tested, rows that agree, rows in front).
 * float32, evaluated exactly as written (no fused operation, correctly rounded division), comparisons false for a
 * NaN: NaN / inf rows, rows behind near_plane, rows outside the image and pixels without depth add nothing.  keep is
 * 1 - rho and beyond 1 + rho, the float32 difference and sum taken by the caller.  The sums are integers: they do not
 * depend on the order of rows, waves or workgroups.  One zeroing launch and one kernel; the number of global atomics
 * is bounded by the kernel's grid cap times 3 n_poses, not by n_rows.
 * Returns GSL_ERR_BAD_ARG before any launch for a NULL means, w2c, depth or counts, n_rows <= 0 or >= 2^31, n_poses
 * outside 1 .. GSL_MAP_SCORE_MAX_POSES (gsl_map_score_max_poses()), width or height <= 0 or width * height > 2^31 - 1,
 * fx or fy not non-zero, keep outside (0, 1], beyond not >= 1. */
#define GSL_MAP_SCORE_MAX_POSES 64
int gsl_map_score_max_poses(void);
int gsl_map_score(const float* means, int64_t n_rows, const float* w2c, int n_poses, float fx, float fy, float cx,
                  float cy, const float* depth, int width, int height, float keep, float beyond, float near_plane,
                  int32_t* counts, void* stream);

/* ---- pose information: the normal equations of a pose from the map's rows against a depth frame (csrc/map_info.hip) ----
 * means[n_rows,3], depth[height,width] float32 (the observed depth, metres) and w2c[16] (world to camera, row-major;
 * twelve entries are read) on the device.  out[GSL_MAP_INFO_VALUES] int64 on the device; it need not be initialised,
 * the entry point zeroes it on the stream.  A left perturbation w2c' = exp(xi^) w2c, xi = (omega [rad], upsilon [m]) in
 * the camera's frame, moves a row's camera point p to p + omega x p + upsilon; against the plane through q0 with unit
 * normal n the residual is r = n . (p - q0) and its derivative J = (p x n, n).  Row i with mean (px, py, pz), w the
 * rows of w2c:
 *   x = ((w0 px + w1 py) + w2 pz) + w3, and y, z likewise;  u = fx x / z + cx, v = fy y / z + cy;
 *   uf = rintf(u), vf = rintf(v) (round half to even);
 *   TESTED when z > near_plane and 1 <= uf <= width - 2 and 1 <= vf <= height - 2 (an inner pixel) and
 *          d0 = depth[vf, uf] is finite and > 0;
 *   lo = d0 * keep, hi = d0 * beyond (one rounded product each);
 *   USED   when tested and z >= lo and z <= hi and z < 64 (what bounds the sums, below) and each of the neighbours
 *          dl, dr, du, dd = depth[vf, uf - 1], depth[vf, uf + 1], depth[vf - 1, uf], depth[vf + 1, uf] is finite and
 *          > 0 with lo <= d <= hi, and the inverse depth is linear across the patch -- with i0 = 1 / d0, s0 = i0 + i0,
 *          tol = kappa * i0: |(1 / dl + 1 / dr) - s0| <= tol and |(1 / du + 1 / dd) - s0| <= tol -- and len > 0;
 *   q(u, v, d) = ((u - cx) / fx * d, (v - cy) / fy * d, d), the back-projection of gsl_map_append;
 *   a = q(uf + 1, vf, dr) - q(uf - 1, vf, dl),  b = q(uf, vf + 1, dd) - q(uf, vf - 1, du),
 *   c = (a.y b.z - a.z b.y, a.z b.x - a.x b.z, a.x b.y - a.y b.x),  len = sqrtf((c.x c.x + c.y c.y) + c.z c.z),
 *   n = c / len;  e = (x, y, z) - q(uf, vf, d0),  r = (n.x e.x + n.y e.y) + n.z e.z,
 *   m = (y n.z - z n.y, z n.x - x n.z, x n.y - y n.x),  J = (m.x, m.y, m.z, n.x, n.y, n.z);
 *   fix(s, t) = llrintf((s * t) * 1048576.f): one float32 product, scaled by 2^20, rounded half to even to an int64.
 *   out[0 .. 20]  = sum of fix(J_a, J_b), a <= b: the upper triangle of H = sum J J^T, row-major;
 *   out[21 .. 26] = sum of fix(J_a, r): g = sum J r;   out[27] = sum of fix(r, r);
 *   out[28] = rows used;  out[29] = rows tested.
 * float32, evaluated exactly as written (no fused operation, correctly rounded division and square root), comparisons
 * false for a NaN: NaN / inf rows, rows at or behind near_plane, rows on the border or outside the image and pixels
 * without depth add nothing.  keep is 1 - rho and beyond 1 + rho, the float32 difference and sum taken by the caller.
 * The sums are integers: they do not depend on the order of rows, waves or workgroups.  The sign of n cancels in every
 * product.  One zeroing launch and one kernel; the number of global atomics is bounded by the kernel's grid cap times
 * GSL_MAP_INFO_VALUES, not by n_rows.  Nothing but out is written.
 * gsl_map_info_max_rows: the rows one call takes, 2^31 - 1 at the most -- under it no sum can leave 64 bits (every
 * |J_a| and |r| is at most B = 64 S (1 + 1 / keep), S^2 = 1 + tx^2 + ty^2 with tx, ty the tangents of the half-angles
 * the inner pixels span; rows < 2^63 / (1.01^2 B^2 2^20 + 1)); 0 for arguments the entry point refuses.
 * Returns GSL_ERR_BAD_ARG before any launch for a NULL means, w2c, depth or out, n_rows <= 0 or >= 2^31 or above
 * gsl_map_info_max_rows, width or height <= 0 or width * height > 2^31 - 1 (an image without an inner pixel is taken:
 * every sum is 0), fx or fy not non-zero, keep outside (0, 1], beyond not in [1, inf), kappa not in [0, inf). */
#define GSL_MAP_INFO_VALUES 30
int gsl_map_info_values(void);
int64_t gsl_map_info_max_rows(float fx, float fy, float cx, float cy, int width, int height, float keep);
int gsl_map_pose_info(const float* means, int64_t n_rows, const float* w2c, float fx, float fy, float cx, float cy,
                      const float* depth, int width, int height, float keep, float beyond, float kappa,
                      float near_plane, int64_t* out, void* stream);

/* ---- pose alignment: Gauss-Newton on the normal equations above, iterated on the device (csrc/map_align.hip) ----
 * means, n_rows, w2c, fx .. near_plane as for gsl_map_pose_info; w2c[16] is the start pose and is not written.
 * sums[GSL_MAP_INFO_VALUES] int64, work[16] float32, state[GSL_MAP_ALIGN_STATE_WORDS] and
 * history[max_steps][GSL_MAP_ALIGN_ROW_WORDS] 8-byte words, all on the device, none of which need be initialised and
 * none of which may overlap another or w2c:
 *   state   = the pose P, the upper 3 x 4 of the world-to-camera matrix row-major as 12 float64 (initially the exact
 *             widening of w2c's 12 float32 entries), then int64 steps_taken (the steps applied), then int64 done;
 *   work    = (float)P, round to nearest even, and the row (0, 0, 0, 1): what the sums of an iteration are taken at;
 *   history = per iteration int64 (status, rows used, rows tested, sum of fix(r, r)), then float64 xi[6] = (omega [rad],
 *             upsilon [m]).
 * One initialising launch; then for each of max_steps iterations the two launches of gsl_map_pose_info at work and a
 * one-thread kernel that, in float64 with one rounding per operation in the order csrc/map_align.hip writes down:
 *   done already: repeats the previous row's status (xi = 0; used, tested and the residual sum are this launch's);
 *   used < min_used: status FEW, done;
 *   solves (H + damping * used * I) xi = -g by LDL^T without pivoting, H and g the sums / 2^20; a pivot that is not
 *     above 0 (a NaN included): status SINGULAR, done;
 *   not (omega . omega <= max_rot^2 and upsilon . upsilon <= max_trans^2): status TOO_FAR (xi is recorded), done;
 *   otherwise P <- [R | upsilon] P with R the Cayley map of omega, ((1 - s) I + 2 a a^T + 2 [a]x) / (1 + s), a = omega
 *     / 2, s = a . a -- an exact rotation that agrees with exp(omega^) to first order and needs no sine or cosine --
 *     work is written, steps_taken goes up by one, and the status is CONVERGED (done) when omega . omega <= eps_rot^2
 *     and upsilon . upsilon <= eps_trans^2, else STEPPED.
 * FEW, SINGULAR and TOO_FAR leave P and work as they were.  The status of the call is that of the last history row.
 * The launches after done cannot be skipped (nothing is read back) and still run.  No allocation, no synchronisation.
 * Returns GSL_ERR_BAD_ARG before any launch for whatever gsl_map_pose_info refuses, a NULL sums, work, state or
 * history, max_steps outside 1 .. GSL_MAP_ALIGN_MAX_STEPS (gsl_map_align_max_steps()), min_used < 7, damping not in
 * [0, inf), max_rot or max_trans not in (0, inf), eps_rot or eps_trans not in [0, inf). */
#define GSL_MAP_ALIGN_MAX_STEPS 32
#define GSL_MAP_ALIGN_STATE_WORDS 14
#define GSL_MAP_ALIGN_ROW_WORDS 10
#define GSL_MAP_ALIGN_STEPPED 0
#define GSL_MAP_ALIGN_CONVERGED 1
#define GSL_MAP_ALIGN_FEW 2
#define GSL_MAP_ALIGN_SINGULAR 3
#define GSL_MAP_ALIGN_TOO_FAR 4
int gsl_map_align_max_steps(void);
int gsl_map_pose_align(const float* means, int64_t n_rows, const float* w2c, float fx, float fy, float cx, float cy,
                       const float* depth, int width, int height, float keep, float beyond, float kappa,
                       float near_plane, int max_steps, double damping, int min_used, double max_rot, double max_trans,
                       double eps_rot, double eps_trans, int64_t* sums, float* work, void* state, void* history,
                       void* stream);

/* ---- pose alignment of several poses in one call, with an early exit per pose (csrc/map_align_batch.hip) ----
 * n_poses (1 .. GSL_MAP_ALIGN_BATCH_MAX_POSES = gsl_map_align_batch_max_poses()) world-to-camera start poses
 * w2c[n_poses][16] are aligned against the same rows, depth frame and parameters, each as gsl_map_pose_align aligns it
 * alone.  The buffers are gsl_map_pose_align's per pose, pose-major, on the device, not initialised, not overlapping:
 * sums[n_poses][GSL_MAP_INFO_VALUES] int64, work[n_poses][16] float32, state[n_poses][GSL_MAP_ALIGN_STATE_WORDS] and
 * history[n_poses][max_steps][GSL_MAP_ALIGN_ROW_WORDS] 8-byte words.
 * One initialising launch; then per iteration a launch that zeroes the sums, one that takes the sums of all poses (the
 * pose on the second grid dimension) and a kernel with one thread per pose that takes gsl_map_pose_align's step.
 * A pose's done word has three values: 0 running; 1 finished, its sums at the final pose still to be taken; 2 closed.
 * A CONVERGED step sets 1: the next iteration takes the sums once more at the pose the step left, records the row (the
 * previous status, xi = 0, as gsl_map_pose_align does after done) and sets 2.  FEW, SINGULAR and TOO_FAR did not move
 * the pose and set 2 at once.  For a closed pose the sums' workgroups leave after reading the word, its 30 sums are not
 * zeroed, and the step kernel repeats the previous row's four integers with xi = 0.
 * For every pose state (done apart), work and every history row are bit for bit what gsl_map_pose_align leaves for that
 * pose alone (it recomputes identical integers at an unchanged pose).  With done == 2, sums[p] are what
 * gsl_map_pose_info gives at work[p]: the normal equations at the final pose.  A pose that converges on the last
 * iteration is left at 1, and its sums are those of the pose before that step.
 * No allocation, no synchronisation, no read-back, no memset node.  Returns GSL_ERR_BAD_ARG before any launch for
 * whatever gsl_map_pose_align refuses and for n_poses outside 1 .. GSL_MAP_ALIGN_BATCH_MAX_POSES. */
#define GSL_MAP_ALIGN_BATCH_MAX_POSES 16
int gsl_map_align_batch_max_poses(void);
int gsl_map_pose_align_batch(const float* means, int64_t n_rows, const float* w2c, int n_poses, float fx, float fy,
                             float cx, float cy, const float* depth, int width, int height, float keep, float beyond,
                             float kappa, float near_plane, int max_steps, double damping, int min_used, double max_rot,
                             double max_trans, double eps_rot, double eps_trans, int64_t* sums, float* work, void* state,
                             void* history, void* stream);

/* ---- a photometric term in the normal equations above, and in the two alignments (csrc/map_photo.hip) ----
 * gsl_map_photo_intensity: rgb[height,width,3] float32 in 0 .. 255 and intensity[height,width] float32 on the device;
 *   intensity[v,u] = ((0.299f R + 0.587f G) + 0.114f B) / 255.f.  One kernel, one thread per pixel: once per frame.
 *   Returns GSL_ERR_BAD_ARG before the launch for a NULL rgb or intensity, width or height <= 0 or width * height >
 *   2^31 - 1.
 * gsl_map_pose_info_photo: gsl_map_pose_info's arguments, then colors[n_rows,3] float32 (the rows' colours, 0 .. 1, as
 *   gsl_map_append stores them), intensity[height,width] (above, of the frame that depth belongs to), photo_scale s
 *   [metres per unit of intensity: how many metres of depth residual one unit of intensity residual is worth] and
 *   photo_max_residual, then extra[2] int64 on the device, not initialised.  A row that is USED -- by the rule above,
 *   untouched -- gives, beside its geometric equation, a photometric one when, with Y the intensity image, c the row's
 *   colour and u, v, uf, vf, x, y, z as above, float32, one rounding per operation in the order written:
 *     Yi = (0.299f c.r + 0.587f c.g) + 0.114f c.b;  Y0, Yl, Yr, Yu, Yd = Y[vf, uf], Y[vf, uf - 1], Y[vf, uf + 1],
 *     Y[vf - 1, uf], Y[vf + 1, uf];  each of the six is >= 0 and <= 1 (false for a NaN);
 *     gx = (Yr - Yl) * 0.5f, gy = (Yd - Yu) * 0.5f;  Yp = (Y0 + gx * (u - uf)) + gy * (v - vf);  rc = Yp - Yi;
 *     |rc| <= photo_max_residual;
 *     a0 = (s * gx) * fx / z, a1 = (s * gy) * fy / z, a2 = -((a0 * x + a1 * y) / z);  every |a_k| <= 8 and z < 16;
 *     Jc = (y a2 - z a1, z a0 - x a2, x a1 - y a0, a0, a1, a2), Jc_6 = s * rc.
 *   out[0 .. 27] are then the sums of fix(J_a, J_b) and of fix(Jc_a, Jc_b) together; out[28] and out[29] keep their
 *   meaning.  extra[0] = the rows that gave a photometric equation, extra[1] = the sum of fix(s rc, s rc) over them.
 *   photo_scale = 0 gives gsl_map_pose_info's 30 integers.  One or two zeroing launches and one kernel; nothing but out
 *   and extra is written.
 * gsl_map_info_photo_max_rows: the rows such a call takes -- with B and S of gsl_map_info_max_rows and
 *   Bc = max(16 S 8 sqrt(3), s photo_max_residual): rows < 2^63 / (1.01^2 (B^2 + Bc^2) 2^20 + 2), 2^31 - 1 at the most; 0
 *   for arguments the entry points refuse.
 * gsl_map_pose_align_photo, gsl_map_pose_align_batch_photo: gsl_map_pose_align and gsl_map_pose_align_batch with these
 *   sums in place of gsl_map_pose_info's in every iteration -- the same launch sequences, state, work and history; the
 *   arguments of the twin, then colors, intensity, photo_scale, photo_max_residual in front of stream.
 * Each returns GSL_ERR_BAD_ARG before any launch, writing nothing, for whatever its twin refuses, a NULL colors,
 * intensity (or extra), photo_scale not in [0, 16], photo_max_residual not in [0, 1], n_rows above
 * gsl_map_info_photo_max_rows. */
int gsl_map_photo_intensity(const float* rgb, int width, int height, float* intensity, void* stream);
int64_t gsl_map_info_photo_max_rows(float fx, float fy, float cx, float cy, int width, int height, float keep,
                                    float photo_scale, float photo_max_residual);
int gsl_map_pose_info_photo(const float* means, int64_t n_rows, const float* w2c, float fx, float fy, float cx, float cy,
                            const float* depth, int width, int height, float keep, float beyond, float kappa,
                            float near_plane, int64_t* out, const float* colors, const float* intensity,
                            float photo_scale, float photo_max_residual, int64_t* extra, void* stream);
int gsl_map_pose_align_photo(const float* means, int64_t n_rows, const float* w2c, float fx, float fy, float cx,
                             float cy, const float* depth, int width, int height, float keep, float beyond, float kappa,
                             float near_plane, int max_steps, double damping, int min_used, double max_rot,
                             double max_trans, double eps_rot, double eps_trans, int64_t* sums, float* work, void* state,
                             void* history, const float* colors, const float* intensity, float photo_scale,
                             float photo_max_residual, void* stream);
int gsl_map_pose_align_batch_photo(const float* means, int64_t n_rows, const float* w2c, int n_poses, float fx, float fy,
                                   float cx, float cy, const float* depth, int width, int height, float keep,
                                   float beyond, float kappa, float near_plane, int max_steps, double damping,
                                   int min_used, double max_rot, double max_trans, double eps_rot, double eps_trans,
                                   int64_t* sums, float* work, void* state, void* history, const float* colors,
                                   const float* intensity, float photo_scale, float photo_max_residual, void* stream);

/* ---- the image pyramid of a frame, for coarse-to-fine alignment (csrc/map_pyramid.hip) ----
 * Level 0 is the frame, depth[height,width] and, when given, intensity[height,width] float32 on the device.  Level l + 1
 * has W' = W / 2, H' = H / 2 (integer division: an odd last column or row is dropped); its pixel (i, j) is made from
 * a, b, c, e = X[2j, 2i], X[2j, 2i+1], X[2j+1, 2i], X[2j+1, 2i+1] of level l, float32, one rounding per operation in the
 * order written, no contraction, correctly rounded division, comparisons false for a NaN:
 *   depth:     valid = each of the four > 0 and < inf, and max * keep <= min;
 *              inv = ((1/a + 1/b) + (1/c + 1/e)) * 0.25f;  d' = 1 / inv where valid, otherwise 0;
 *   intensity: Y' = ((a + b) + (c + e)) * 0.25f, unconditionally.
 * The intrinsics of level l + 1 are the caller's, in float32: fx' = fx * 0.5f, fy' = fy * 0.5f, cx' = (cx - 0.5f) *
 * 0.5f, cy' = (cy - 0.5f) * 0.5f (pixel u lies at the integer u, the centre of a block at 2i + 0.5).
 * gsl_map_pyramid_floats: the floats of levels 1 .. levels packed one after another, each row-major; 0 for arguments
 *   gsl_map_pyramid refuses.
 * gsl_map_pyramid: depth_out and, with an intensity, intensity_out hold that many floats on the device, not initialised,
 *   overlapping nothing; every one of them is written exactly once and nothing else is.  One kernel, a workgroup per 32 x
 *   32 tile of level 0; no zeroing launch, no atomics, no allocation, no synchronisation.  intensity and intensity_out
 *   are both NULL (depth only) or both given.  Returns GSL_ERR_BAD_ARG before the launch for a NULL depth or depth_out,
 *   one of the intensity pair without the other, width or height <= 0 or width * height > 2^31 - 1, levels outside 1 ..
 *   GSL_MAP_PYRAMID_MAX_LEVELS, keep not in (0, 1], a coarsest level smaller than 4 x 4.
 * Nothing changes in gsl_map_pose_info* and gsl_map_pose_align*: they take width, height, the intrinsics and the images
 * per call, and a level is another call. */
#define GSL_MAP_PYRAMID_MAX_LEVELS 4
int64_t gsl_map_pyramid_floats(int width, int height, int levels);
int gsl_map_pyramid(const float* depth, const float* intensity, int width, int height, int levels, float keep,
                    float* depth_out, float* intensity_out, void* stream);

/* ---- exposure compensation for the photometric term: an affine brightness model per frame (csrc/map_exposure.hip) ----
 * gain and offset with gain * Y_frame + offset ~ Y_row over the rows of the map that the frame sees, estimated on the
 * device by least squares, and applied to the frame's rgb: Y(gain * rgb + 255 * offset) = gain * Y(rgb) + offset.
 * gsl_map_exposure_estimate: means[n_rows,3], colors[n_rows,3] (0 .. 1), w2c[16], fx .. cy, depth[height,width] and
 *   intensity[height,width] (gsl_map_photo_intensity of the frame) as for gsl_map_pose_info_photo.  On the device, not
 *   initialised, not overlapping: sums[GSL_MAP_EXPOSURE_VALUES] int64, params[4] float32 = (gain, offset, 255 * offset,
 *   0) and record[passes][GSL_MAP_EXPOSURE_RECORD_WORDS] 8-byte words, per pass int64 (status, rows used, rows seen), then
 *   float64 (g, b, rss).  One initialising launch, params = (1, 0, 0, 0); then per pass a zeroing launch, the sums and a
 *   one-thread kernel.  Per row, float32, one rounding per operation in the order written, comparisons false for a NaN:
 *     seen = z > near_plane and 0 <= uf <= width - 1 and 0 <= vf <= height - 1 and d0 = depth[vf, uf] > 0 and < inf and
 *            d0 * keep <= z <= d0 * beyond (the nearest pixel only: border pixels count);
 *     Yi = (0.299f c.r + 0.587f c.g) + 0.114f c.b;  Y0 = intensity[vf, uf];
 *     used = seen and sat_lo <= Yi, Y0 <= sat_hi and |(params[0] * Y0 + params[1]) - Yi| <= gate, gate +inf in the first
 *            pass and max_residual afterwards;
 *     sums = sum fix(Y0, Y0), fix(Y0, 1), fix(Y0, Yi), fix(Yi, 1), fix(Yi, Yi), rows used, rows seen, fix as above.
 *   The one-thread kernel, in float64 with one rounding per operation in the order csrc/map_exposure.hip writes down:
 *     a pass before this one was not OK: its status is repeated, g, b = params, rss = 0;
 *     used < min_used: FEW;  det = n Sxx - Sx Sx, not (det / (n n) > min_var): FLAT (both: g, b = params, rss = 0);
 *     g = (n Sxy - Sx Sy) / det, b = (Sy - g Sx) / n, rss = (Syy - g Sxy) - b Sy;
 *     not (gain_min <= g <= gain_max and |b| <= offset_max): RANGE;  otherwise OK and params = ((float)g, (float)b,
 *     (float)b * 255.f, 0).  Every status but OK leaves params as they were; the later passes still run and change
 *     nothing but their record.  The status of the call is that of the last record.
 *   No allocation, no synchronisation, no read-back, no memset node, no float atomics.  Returns GSL_ERR_BAD_ARG before
 *   any launch for a NULL pointer, n_rows <= 0 or >= 2^31, width or height <= 0 or width * height > 2^31 - 1, fx or fy
 *   not non-zero, keep outside (0, 1], beyond not in [1, inf), not 0 <= sat_lo < sat_hi <= 1 (what keeps every term of a
 *   sum at 2^20 or less, every sum below 2^51), max_residual not in [0, inf), passes outside 1 ..
 *   GSL_MAP_EXPOSURE_MAX_PASSES, min_used < 1, not 0 < gain_min <= 1 <= gain_max < inf, offset_max or min_var not in
 *   [0, inf).
 * gsl_map_exposure_apply: rgb[height,width,3] and out (the same size, not overlapping it) float32 on the device, params
 *   as above: t = (params[0] * c) + params[2];  out = 0 where t < 0, 255 where t > 255, t otherwise (a NaN stays one).
 *   One kernel, one thread per value.  Returns GSL_ERR_BAD_ARG before the launch for a NULL pointer or such a size. */
#define GSL_MAP_EXPOSURE_VALUES 7
#define GSL_MAP_EXPOSURE_RECORD_WORDS 6
#define GSL_MAP_EXPOSURE_MAX_PASSES 4
#define GSL_MAP_EXPOSURE_OK 0
#define GSL_MAP_EXPOSURE_FEW 1
#define GSL_MAP_EXPOSURE_FLAT 2
#define GSL_MAP_EXPOSURE_RANGE 3
int gsl_map_exposure_values(void);
int gsl_map_exposure_estimate(const float* means, const float* colors, int64_t n_rows, const float* w2c, float fx,
                              float fy, float cx, float cy, const float* depth, const float* intensity, int width,
                              int height, float keep, float beyond, float near_plane, float sat_lo, float sat_hi,
                              float max_residual, int passes, int min_used, double gain_min, double gain_max,
                              double offset_max, double min_var, int64_t* sums, float* params, void* record,
                              void* stream);
int gsl_map_exposure_apply(const float* rgb, int width, int height, const float* params, float* out, void* stream);

/* ---- place recognition: a 16 x 12 descriptor of a depth frame, and its match against keyframes (csrc/map_place.hip) ----
 * gsl_map_place_describe: depth[height,width] float32 on the device, row-major, metres; desc[192] int32 on the device,
 * row-major over GSL_MAP_PLACE_GH lines of GSL_MAP_PLACE_GW cells (gsl_map_place_cells() = 192).  It need not be
 * initialised: every entry is written by the one workgroup that owns its cell, nothing is accumulated in global memory.
 *   Pixel (u, v) belongs to cell ((u * 16) / width, (v * 12) / height), integer division.
 *   A pixel counts when d > 0 and d < inf (both false for a NaN): its value is
 *     q = (uint32) rintf(fminf(d, 63.f) * 1024.f) -- one rounded float32 product, round half to even, at most 64 512.
 *   desc[cell] = sum(q) / count (floored integer division) when count > 0 and 2 count >= the pixels of the cell;
 *     otherwise -1 (invalid).
 * Everything after q is integer arithmetic: the result does not depend on the order of pixels, waves or workgroups.
 * One kernel; no atomics on global memory.
 * Returns GSL_ERR_BAD_ARG before any launch for a NULL depth or desc, width < 16 or height < 12, or an image whose
 * largest cell, ceil(width / 16) x ceil(height / 12) pixels, holds more than 65 536 (its sum would leave 32 bits).
 *
 * gsl_map_place_match: query[192] and table[n_keyframes,192] int32 on the device, descriptors as above (an entry is
 * valid when it is >= 0); out[n_keyframes,15,2] int32 on the device, written whole.  The 15 shifts (sx, sy), sx in
 * -2 .. 2 and sy in -1 .. 1, are numbered s = (sy + 1) * 5 + (sx + 2): sy-major, both ascending.  For keyframe k and
 * shift s, over the cells (i, j) with 0 <= i + sx < 16 and 0 <= j + sy < 12 at which query[(j + sy) * 16 + i + sx] and
 * table[k][j * 16 + i] are both valid:
 *   out[k][s][0] = common, the number of those cells;
 *   out[k][s][1] = sum, the sum of |query[(j + sy) * 16 + i + sx] - table[k][j * 16 + i]| over them (<= 192 x 64 512).
 * Integers: the same on every run.  One kernel, one 64-lane wave per (keyframe, shift).
 * Returns GSL_ERR_BAD_ARG before any launch for a NULL query, table or out, or n_keyframes outside
 * 1 .. GSL_MAP_PLACE_MAX_KEYFRAMES. */
#define GSL_MAP_PLACE_GW 16
#define GSL_MAP_PLACE_GH 12
#define GSL_MAP_PLACE_MAX_KEYFRAMES 256
int gsl_map_place_cells(void);
int gsl_map_place_describe(const float* depth, int width, int height, int32_t* desc, void* stream);
int gsl_map_place_match(const int32_t* query, const int32_t* table, int n_keyframes, int32_t* out, void* stream);

/* ---- refinement: the rows a depth frame observes again move to the running mean of their depths (csrc/map_refine.hip) ----
 * means[n_rows,3] and colors[n_rows,3] float32 and weights[n_rows] int32 on the device, as in the map: weights[i] >= 1
 * is the number of depths row i is the mean of.  depth[height,width] float32 (the observed depth, metres) and
 * rgb[height,width,3] float32 in 0..255, row-major, on the device; w2c[16] (world to camera, row-major, on the device;
 * twelve entries are read); cam_x, cam_y, cam_z: the camera centre in the world.  counters is int32[1]; it need not be
 * initialised, the entry point zeroes it on the stream.  Row i with mean p, colour c and weight w:
 *   x = ((w0 px + w1 py) + w2 pz) + w3, and y, z likewise from rows 1 and 2 of w2c;
 *   u = fx x / z + cx, v = fy y / z + cy;
 *   CANDIDATE when z > near_plane and 0 <= u <= width - 1 and 0 <= v <= height - 1 (on u and v, not on rounded values);
 *   u0 = min((int)floorf(u), width - 2), v0 = min((int)floorf(v), height - 2), a = u - (float)u0, b = v - (float)v0:
 *             a row on the last column or line has a == 1 or b == 1 and reads pixels inside the image only;
 *   d00, d10, d01, d11 = depth at (u0, v0), (u0 + 1, v0), (u0, v0 + 1), (u0 + 1, v0 + 1);
 *   REFINED   when candidate and each of the four is finite and > 0 with z >= d * keep and z * keep <= d (the
 *             predicate of gsl_map_observe, both ways).  Every other row keeps every bit of its mean, colour and weight;
 *   BLEND     a1 = 1 - a, b1 = 1 - b, w00 = a1 * b1, w10 = a * b1, w01 = a1 * b, w11 = a * b,
 *             blend(x00, x10, x01, x11) = ((w00 * x00 + w10 * x10) + w01 * x01) + w11 * x11;
 *   d  = 1 / blend(1 / d00, 1 / d10, 1 / d01, 1 / d11): the inverse depth of a plane is linear in the pixel, so on a
 *             planar patch d is the depth on the row's own ray up to rounding, wherever in the pixel it projects;
 *   wf = (float)(w + 1) (the sum taken in 64 bits),  t = (d - z) / (z * wf);
 *   mean      p' = p + (p - cam) * t per component (one product and one sum each): along the row's ray, to the running
 *             mean of its depths; d == z leaves p as it is;
 *   colour    c' = c + (blend(rgb / 255.f at the four pixels, per channel) - c) / wf, when rgb is given;
 *   weight    w' = min(w + 1, max_weight): at the cap the mean goes on as an exponential one, gain 1 / (max_weight + 1);
 *   counters[0] = rows refined (an integer sum: it does not depend on the order of rows, waves or workgroups).
 * float32, evaluated exactly as written (no fused operation, correctly rounded division), comparisons false for a NaN:
 * NaN / inf rows, rows at or behind near_plane, rows outside the image and rows with a pixel without depth among their
 * four are left alone.  keep is 1 - rho, the float32 difference taken by the caller.  In place: a thread reads and
 * writes its own row only.  colors and rgb come together, or both are NULL and the colours are left alone.  One zeroing
 * launch and one kernel; the number of global atomics is bounded by the kernel's grid cap, not by n_rows.
 * Returns GSL_ERR_BAD_ARG before any launch for a NULL means, weights, w2c, depth or counters, colors without rgb or
 * rgb without colors, n_rows <= 0 or >= 2^31, width or height < 2 or width * height > 2^31 - 1, fx or fy not non-zero,
 * keep outside (0, 1], a camera centre that is not finite, max_weight outside 1 .. 2^30. */
int gsl_map_refine(float* means, float* colors, int32_t* weights, int64_t n_rows, const float* w2c, float cam_x,
                   float cam_y, float cam_z, float fx, float fy, float cx, float cy, const float* depth,
                   const float* rgb, int width, int height, float keep, float near_plane, int max_weight,
                   int32_t* counters, void* stream);

/* ---- trajectory correction: the rows follow the frame they came from (csrc/map_correct.hip) ----
 * means[n_rows,3] float32 and origins[n_rows] int32 on the device, as in the map: origins[i] is the index, in the
 * trajectory, of the frame that appended row i.  table[n_frames,12] float32 on the device: per frame a row-major 3 x 4
 * [R | t], the rigid transform of the world that takes the frame's old pose to its corrected one.  counters is
 * int64[2]; it need not be initialised, the entry point zeroes it on the stream.  Row i with mean (x, y, z),
 * o = origins[i] and e = table[12 o .. 12 o + 11]:
 *   OUTSIDE   when o < 0 or o >= n_frames;
 *   MOVED     when not outside, x, y and z are finite, and e is not the identity: some of the twelve comparisons
 *             e0 == 1, e1 == 0, e2 == 0, e3 == 0, e4 == 0, e5 == 1, e6 == 0, e7 == 0, e8 == 0, e9 == 0, e10 == 1,
 *             e11 == 0 is false (-0.0 counts as 0);
 *   a moved row becomes  x' = ((e0 x + e1 y) + e2 z) + e3,  y' = ((e4 x + e5 y) + e6 z) + e7,
 *             z' = ((e8 x + e9 y) + e10 z) + e11;
 *   every other row keeps every bit of its mean: a NaN or inf row, a -0.0 coordinate under an identity entry, an
 *             origin outside the table.  Only the means are ever written;
 *   counters[0] = rows moved, counters[1] = rows outside (integer sums: they do not depend on the order of rows, waves
 *             or workgroups).
 * float32, evaluated exactly as written (one rounding per operation, no fused operation), comparisons false for a NaN.
 * In place: a thread reads and writes its own row only.  One zeroing launch and one kernel; the number of global
 * atomics is bounded by the kernel's grid cap, not by n_rows.  n_rows == 0 is GSL_OK without a launch (the counters
 * are then not touched).
 * Returns GSL_ERR_BAD_ARG before any launch for a NULL means, origins, table or counters, n_frames < 1, n_rows < 0 or
 * >= 2^31. */
int gsl_map_correct(float* means, const int32_t* origins, int64_t n_rows, const float* table, int n_frames,
                    int64_t* counters, void* stream);

/* ---- covisibility: the verdicts of the pose scores, binned by the frame a row came from (csrc/map_covis.hip) ----
 * means[n_rows,3] float32 and origins[n_rows] int32 on the device, as in the map; w2c[16] (world to camera, row-major;
 * twelve entries are read) and depth[height,width] float32 (the observed depth, metres) on the device.
 * counts[n_frames,3] int32 and outside[1] int64 on the device; they need not be initialised, the entry point zeroes them
 * on the stream.  Row i with o = origins[i] -- the origin is looked at first:
 *   OUTSIDE when o < 0 or o >= n_frames: outside[0] += 1 and nothing else, whatever the row's mean is;
 *   otherwise TESTED, AGREE, FRONT and BEHIND are those of gsl_map_score for the one pose w2c, operation for operation
 *           (above: the projection, the row's own pixel, keep and beyond, comparisons false for a NaN), and
 *   counts[o] += (tested, agree, front).
 * The sums are integers: they do not depend on the order of rows, waves or workgroups, nor on the order of the
 * origins -- a map has them non-decreasing, which the kernel uses for speed only.  The sum of counts over the frames is
 * what gsl_map_score leaves for the same pose whenever no row is outside.  Two zeroing launches and one kernel; a
 * workgroup combines its waves over a window of 64 consecutive origins before it adds to counts, a run of equal origins
 * outside that window is added with one integer atomic per non-zero predicate; no atomic per row.  n_rows == 0 is
 * GSL_OK without a launch (counts and outside are then not touched).
 * Returns GSL_ERR_BAD_ARG before any launch for a NULL means, origins, w2c, depth, counts or outside, n_frames outside
 * 1 .. GSL_MAP_COVIS_MAX_FRAMES, n_rows < 0 or >= 2^31, width or height <= 0 or width * height > 2^31 - 1, fx or fy not
 * non-zero, keep outside (0, 1], beyond not >= 1. */
#define GSL_MAP_COVIS_MAX_FRAMES 16777216
int gsl_map_covis(const float* means, const int32_t* origins, int64_t n_rows, const float* w2c, float fx, float fy,
                  float cx, float cy, const float* depth, int width, int height, float keep, float beyond,
                  float near_plane, int n_frames, int32_t* counts, int64_t* outside, void* stream);

/* ---- spherical harmonics: gsplat.spherical_harmonics fwd/bwd (IDX:14306, IDX:14297) ----
 * dirs[M,3], coeffs[M,K,3] with K >= (degree+1)^2, masks[M] (uint8, may be NULL).
 * degree 0..3.  v_dirs may be NULL. */
int gsl_sh_fwd(int degree, const float* dirs, const float* coeffs, const uint8_t* masks, int M,
               int K, float* colors, void* stream);
int gsl_sh_bwd(int degree, const float* dirs, const float* coeffs, const uint8_t* masks, int M,
               int K, const float* v_colors, float* v_coeffs, float* v_dirs, void* stream);

/* ---- tile binning: gsplat.isect_tiles + isect_offset_encode (IDX:14360, IDX:14369) ----
 * Tiles are tile_size x tile_size pixels; tile rows [ty0, ty1) of the tile_w x tile_h grid
 * are binned (ty0=0, ty1=tile_h for the whole image; a strip for tile-parallel ranks).
 * Tile ids in keys and offsets are GLOBAL (ty*tile_w+tx).
 *
 * gsl_isect_count: tiles_per_gauss[N] (may be NULL), tile_offsets[n_tiles+1] exclusive scan over
 *   all tile_w*tile_h tiles (tiles outside the strip are empty), n_isects[1] = total.
 *   ws: gsl_isect_ws_bytes(tile_w*tile_h).
 * gsl_isect_fill: after gsl_isect_count with the same arguments.  Writes, for every tile,
 *   its intersections sorted by (float32 depth bits, Gaussian index) ascending:
 *   flatten_ids[I] and, if not NULL, isect_ids[I] = (cam_id << (32+tile_n_bits)) | (tile_id << 32) | depth bits.
 *   sort_keys[capacity] is scratch (8 bytes per intersection).  Intersections with
 *   position >= capacity are dropped (caller compares n_isects with capacity). */
size_t gsl_isect_ws_bytes(int n_tiles);
int gsl_isect_count(const float* means2d, const int32_t* radii, int N, int tile_size, int tile_w,
                    int tile_h, int ty0, int ty1, int32_t* tiles_per_gauss, int32_t* tile_offsets,
                    int32_t* n_isects, void* ws, size_t ws_bytes, void* stream);
int gsl_isect_fill(const float* means2d, const int32_t* radii, const float* depths, int N,
                   int tile_size, int tile_w, int tile_h, int ty0, int ty1, int cam_id,
                   int tile_n_bits, const int32_t* tile_offsets, int64_t capacity,
                   uint64_t* sort_keys, int32_t* flatten_ids, int64_t* isect_ids, void* ws,
                   size_t ws_bytes, void* stream);

/* Sort every tile bucket of tiles [tile_begin, tile_begin+n_strip_tiles) on (depth bits, id) and
 * write flatten_ids / isect_ids (second half of gsl_isect_fill; cam_enc is OR-ed into isect_ids).
 * Keys are (float32 depth bits << 32) | id with 0 <= id < 2^31 and a depth from +0.0 to +inf (sign bit clear, not
 * NaN; see "Sort keys" below): a negative, -0.0 or NaN depth gets an order that depends on the list length.
 * gsl_isect_fill takes the same depths.  Positions >= capacity are dropped: a tile's span is cut at capacity, later
 * entries are left untouched.
 * The environment variable GSL_DEV_TILE_SORT (read on every call; development and tests) picks the kernel:
 * "wg" = one tile per workgroup (k_tile_sort_wg), "wave16" / "wave32" = one tile per wave with up to 16 / 32 keys
 * per lane (k_tile_sort<4> / <5>), "wave" = one tile per wave, keys per lane by the mean list length; unset or any
 * other value = the library's choice.  Every kernel gives the same result. */
int gsl_tile_sort(const int32_t* tile_offsets, int tile_begin, int n_strip_tiles, int64_t capacity,
                  uint64_t* sort_keys, int32_t* flatten_ids, int64_t* isect_ids, int64_t cam_enc,
                  void* stream);

/* Unsorted emit in Gaussian order (isect_tiles(sort=False)): cum_tiles[N] is the
 * INCLUSIVE cumulative sum of tiles_per_gauss (int64). */
int gsl_isect_emit(const float* means2d, const int32_t* radii, const float* depths,
                   const int64_t* cum_tiles, int N, int tile_size, int tile_w, int tile_h,
                   int cam_id, int tile_n_bits, int id_offset, int64_t* isect_ids,
                   int32_t* flatten_ids, void* stream);

/* Tile start offsets from sorted keys (isect_offset_encode): offsets[n_cameras*n_tiles]. */
int gsl_isect_offsets(const int64_t* isect_ids, int64_t n_isects, int n_cameras, int n_tiles,
                      int tile_n_bits, int32_t* offsets, void* stream);

/* ---- compositing: gsplat.rasterize_to_pixels fwd/bwd (IDX:14378, IDX:14279) ----
 * One camera.  channels in {1,2,3,4,5,8,16,32}.  tile_offsets[n_tiles+1] (global tile ids),
 * flatten_ids index the per-Gaussian arrays directly.  Rows of tile rows [ty0,ty1) are
 * rendered into full-size images (pixels outside the strip are left untouched).
 * backgrounds[channels] may be NULL.
 * t_final[height*width] (may be NULL): the transmittance T every pixel ends with, as the forward holds it.
 * render_alphas is 1 - T rounded to float32, and 1 - render_alphas keeps no more than 2^-24 absolute of T: behind
 * many thin layers (T near the 1e-4 stop) that is 3e-4 relative, and every gradient term of the pixel scales with it.
 * A backward given t_final starts from T itself; given NULL it starts from 1 - render_alphas. */
int gsl_rasterize_fwd(const float* means2d, const float* conics, const float* colors,
                      const float* opacities, const float* backgrounds, int channels, int width,
                      int height, int tile_size, int tile_w, int tile_h, int ty0, int ty1,
                      const int32_t* tile_offsets, const int32_t* flatten_ids, int64_t capacity,
                      float* render_colors, float* render_alphas, int32_t* last_ids, float* t_final,
                      void* stream);

/* vjp.  Per-Gaussian gradients are ACCUMULATED INTO `vacc`, one padded row per Gaussian:
 * [v_means2d 2][v_conics 3][v_opacity 1][v_colors channels], row pitch 16 floats for
 * channels <= 10 and 48 floats otherwise (gsl_vacc_bytes gives the size).  The caller zeroes
 * vacc before the first camera; rows are indexed by the same ids as flatten_ids.
 * gsl_vacc_unpack splits the rows into the four gsplat gradient tensors.
 * t_final (may be NULL): what gsl_rasterize_fwd wrote for this camera, see there. */
size_t gsl_vacc_bytes(int n_gaussians, int channels);
int gsl_rasterize_bwd(const float* means2d, const float* conics, const float* colors,
                      const float* opacities, const float* backgrounds, int channels, int width,
                      int height, int tile_size, int tile_w, int tile_h, int ty0, int ty1,
                      const int32_t* tile_offsets, const int32_t* flatten_ids, int64_t capacity,
                      const float* render_alphas, const int32_t* last_ids, const float* t_final,
                      const float* v_render_colors, const float* v_render_alphas, float* vacc,
                      void* stream);
int gsl_vacc_unpack(const float* vacc, int n_gaussians, int channels, float* v_means2d,
                    float* v_conics, float* v_colors, float* v_opacities, void* stream);

/* ---- fused single-camera pipeline: gsplat.rasterization end to end (IDX:14954) ----
 * The hot path of GsplatLoc's tracker (model.py:195-213).  16x16 tiles.  Per-Gaussian state lives
 * in 16-byte records: Q0[N] = (x, y, depth, opacity_eff), Q1[N] = (conic a, b, c, r_cull),
 * Q2[N] = (r, g, b, 0) (NULL for depth-only rendering).  channels: 1 = depth, 3 = RGB,
 * 4 = RGB + depth; ed != 0 divides the depth channel by alpha (render modes "ED"/"RGB+ED").
 * colors: SH coefficients [N,K_sh,3] when sh_degree in 0..3, direct RGB [N,3] when sh_degree < 0.
 * ws: gsl_fused_ws_bytes(N, tile_w*tile_h), shared by the five calls of one render.
 *
 * gsl_fused_project : projection + colour + pack + tile histogram + scan
 *                     -> radii, Q0, Q1, Q2, tile_offsets[n_tiles+1], n_isects[1]
 * gsl_fused_bin     : scatter + per-tile sort -> flatten_ids (isect_ids optional)
 * gsl_fused_raster_fwd / _bwd : compositing and its vjp; the vjp ACCUMULATES into vacc, 16 floats
 *                     per Gaussian ([v_xy 2][v_conic 3][v_opacity 1][v_colour channels]), zero on entry.
 *                     Forward: every lane walks the candidate list of its own pixel (csrc/raster_px.hip);
 *                     backward: each 16-lane DPP row of a wave walks the list of its own 4x4 pixel block
 *                     (csrc/raster_g16.hip; deterministic mode: quadrant walk with per-splat pixel sums on the
 *                     matrix cores, v_mfma_f32_16x16x4_f32, exact f32, csrc/fused.hip).  isect_hits (uint32[4 x capacity])
 *                     + isect_hit_counts (int32[4 x n_tiles + 1]), may be NULL together in both calls: the forward leaves, per
 *                     tile and 8x8 quadrant, the list of the entries at least one of the quadrant's pixels composited --
 *                     (nibble of its four 4x4 blocks that did) << 28 | list index, in list order, at
 *                     isect_hits[4 start + quadrant x length ...] for the tile's list [start, start + length), its
 *                     length in isect_hit_counts[4 tile + quadrant] (the extra last int is a flag between the
 *                     backward's two launches) -- and the backward given the same arrays walks
 *                     exactly those (block, entry) pairs instead of scanning the tile's list and testing every splat's
 *                     alpha >= 1/255 disc against the blocks.  (Segments of long lists: same layout per segment, the
 *                     lengths live in long_ws.)  Only pixel rows [row0,row1)
 *                     of the tile rows [ty0,ty1) are rendered / back-propagated (whole strip: 0,height):
 *                     a strip's one-pixel Sobel halo costs one pixel row, not a tile row.
 * fp16 staging (Qh, may be NULL everywhere): gsl_fused_project additionally packs one 32-byte record per Gaussian
 *                     into Qh[N][8 dwords] -- centre float32, conic / cull radius / depth / opacity / colour as
 *                     halves -- and the compositing calls given Qh gather that record instead of Q0/Q1/Q2 (which may
 *                     then be NULL there; gsl_fused_project given Qh does not write Q2 at all).  Transmittance and every accumulator stay float32 (BASELINE.json
 *                     configs[4] "fp16 compositing").  Binning and gsl_fused_project_bwd keep reading
 *                     the float32 records, so the list order is the float32 order.
 * Deterministic mode (vrow, may be NULL): by default the backward accumulates with float atomics (LDS across the
 *                     four waves of a tile, memory across the tiles of a Gaussian), whose order varies from run to
 *                     run.  With write_sorted_keys = 1 in gsl_fused_bin (sort_keys then holds the sorted
 *                     (depth bits << 32 | id) keys) and vrow[capacity][16] given to gsl_fused_raster_bwd (vacc may be
 *                     NULL) and gsl_fused_project_bwd (with sorted_keys, tile_offsets, Q0 and the strip), every sum
 *                     has a fixed order: waves in wave order, a Gaussian's tiles in tile order (its entry in a tile
 *                     list is found by binary search).  Bit-identical gradients run to run.
 * Binned mode (bins, may be NULL): when the caller knows an upper bound of a tile's list length (a tracker renders the
 *                     same Gaussians hundreds of times per frame), gsl_fused_project given bins[n_tiles][bin_cap]
 *                     (uint64) writes every (depth bits << 32 | id) key straight into its tile's bin and leaves
 *                     the tile sizes in ws (it does NOT write tile_offsets / n_isects then); gsl_fused_bin given the
 *                     same bins adds the sizes up inside its sort kernel -- tile_offsets[n_tiles + 1] and n_isects
 *                     are its OUTPUTS in this mode -- and sorts; gsl_fused_raster_fwd given binned_ws = ws clears
 *                     the counters for the next projection.  The three calls belong together: the scatter pass,
 *                     its second read of the records, the scan launch and the counter-clearing launch disappear.
 *                     ws must be zero-filled once before the first call.  A tile that outgrows bin_cap keeps its
 *                     first bin_cap entries, raises flags[1] = 1 and leaves the largest count in flags[2]
 *                     (flags: 4 ints, may be NULL): poll it and re-run with larger bins.  Counter contract: the
 *                     counters in ws must be zero when gsl_fused_project starts; gsl_fused_raster_fwd(binned_ws = ws)
 *                     leaves them so.  A projection that follows another one without a compositing forward in
 *                     between (skipped, or failed) finds the state word in ws dirty and raises flags[3] = 1: zero-fill
 *                     ws and run the iteration again.
 * Tile-order placement (order_ids / storage_of, int32[N] each, may be NULL together everywhere): a caller that renders the
 *                     same Gaussians many times (a tracker: /root/reference/src/my_gsplat/model.py:137-175 builds them
 *                     once per frame) may STORE them sorted by the tile of their centre, so that the record gathers of a
 *                     tile's list touch a few contiguous runs.  The list order must not depend on the placement -- depth
 *                     ties break by Gaussian index -- so gsl_fused_project (and gsl_fused_bin's scatter pass) put
 *                     order_ids[slot], the Gaussian's ORIGINAL index, into the low key word, and every sort
 *                     (gsl_fused_bin, gsl_long_sort, the sorting gsl_fused_raster_fwd) writes storage_of[original] into
 *                     flatten_ids: the lists are the unpermuted run's lists with every id relabelled, images and
 *                     last_ids bit-identical.  Everything per Gaussian (records, vacc, v_means ...) is then in storage
 *                     order.  Not with write_sorted_keys (the deterministic backward searches the keys by id).
 * Sort keys: (depth bits << 32) | Gaussian index, the depth a positive finite normal float -- gsl_fused_project and
 *                     gsl_project_fwd clamp their depth window to [FLT_MIN, FLT_MAX], so every key this library makes is
 *                     one; the per-tile sorts (gsl_fused_bin, gsl_tile_sort_keys, gsl_long_sort, the sorting forward)
 *                     compare keys partly as doubles and partly as unsigned integers.  The two orders agree for every
 *                     depth from +0.0 to +inf (the high word stays below 0x7FF00000, a double's inf / NaN) and for no
 *                     other: depths handed to the stage-wise isect entry points must be such (gsplat.isect_tiles raises
 *                     ValueError for a visible Gaussian with a negative, -0.0 or NaN depth).
 * Limits: N <= 2^26 Gaussians per call (gsl_fused_project returns GSL_ERR_BAD_ARG beyond: the compositing backward
 *                     addresses the 64-byte gradient rows of vacc by 32-bit byte offsets).
 * gsl_fused_project_bwd : consumes AND CLEARS vacc (gsl_fused_project_bwd_keep: consumes it and leaves it); v_means/v_quats/v_scales/v_opacities (and
 *                     v_colors, shaped like colors) may be NULL together (pose-only);
 *                     v_viewmat[16] is overwritten (row 3 = 0).  tiny_trec / tiny_vcT (may be NULL): the slabs
 *                     gsl_tiny_raster_bwd filled; the kernel then folds them itself (pass 2 of the tiny-splat
 *                     backward fused in: the gradient rows never leave LDS, vacc is not touched, Q0 required)
 *                     instead of reading vacc.  reduce_viewmat = 0 skips that last reduction
 *                     launch and leaves the pose gradient as ceil(N/256) partial rows of 16 floats at
 *                     gsl_fused_viewmat_rows(ws, n_tiles) for gsl_pose_step / gsl_pack_pose_reduce to sum
 *                     (same fixed order, same result; v_viewmat may then be NULL). */
size_t gsl_fused_ws_bytes(int N, int n_tiles);
int gsl_fused_project(const float* means, const float* quats, const float* scales,
                      const float* opacities, const float* colors, int sh_degree, int K_sh,
                      const float* viewmat, const float* K, int N, int width, int height,
                      float eps2d, float near_plane, float far_plane, float radius_clip,
                      int antialiased, int tile_w, int tile_h, int ty0, int ty1, int32_t* radii,
                      float* Q0, float* Q1, float* Q2, float* compensations,
                      int32_t* tiles_per_gauss, int32_t* tile_offsets, int32_t* n_isects, void* ws,
                      size_t ws_bytes, void* Qh, void* bins, int bin_cap, int32_t* flags,
                      const int32_t* order_ids, void* stream);
int gsl_fused_bin(const float* Q0, const int32_t* radii, int N, int tile_w, int tile_h, int ty0,
                  int ty1, int tile_n_bits, int32_t* tile_offsets, int64_t capacity,
                  uint64_t* sort_keys, int32_t* flatten_ids, int64_t* isect_ids, void* ws,
                  size_t ws_bytes, int write_sorted_keys, void* bins, int bin_cap, int32_t* n_isects,
                  int32_t* flags, int long_min, const int32_t* order_ids, const int32_t* storage_of, void* stream);
/* Who clears the gradient rows.  The compositing backward adds into vacc and must find it zero.  By default
 * gsl_fused_project_bwd restores that: it clears every row it has read -- 48 bytes of zero stores per visible Gaussian
 * in the one kernel of the step that runs at what the memory system gives.  A caller that renders again and again (a
 * context with preallocated buffers) can move the clearing into the sort launch of the NEXT forward, whose memory pipes
 * are idle while its waves run their sorting networks:
 *   gsl_fused_bin_clear        = gsl_fused_bin, and the same launch zeroes rows[N][16] (all of it, contiguously, split
 *                                over the launch's waves / workgroups whatever their number; every kernel behind the
 *                                sort, binned or two-pass, whole frame or strip).  rows must not be NULL when N > 0.
 *                                Where gsl_fused_bin would return without a sort launch (capacity 0, an empty strip)
 *                                the rows are zeroed by a launch of their own: after GSL_OK they are zero.
 *   gsl_fused_project_bwd_keep = gsl_fused_project_bwd on the general path (vacc required; vrow and tiny_trec must be
 *                                NULL), reading the rows and leaving them as they are.
 *   gsl_fused_clear_rows       : zeroes rows[N][16] with a kernel of the library (not a memset node: see
 *                                csrc/misc.hip) -- for the caller that runs a second backward after one forward and
 *                                so finds the rows of a _keep call still standing.
 * The invariant is unchanged -- zero rows when a compositing backward starts -- and the caller keeps track of who owes
 * the clearing (gsplatloc_amd/context.py: RenderContext._rows_dirty). */
int gsl_fused_bin_clear(const float* Q0, const int32_t* radii, int N, int tile_w, int tile_h, int ty0,
                        int ty1, int tile_n_bits, int32_t* tile_offsets, int64_t capacity,
                        uint64_t* sort_keys, int32_t* flatten_ids, int64_t* isect_ids, void* ws,
                        size_t ws_bytes, int write_sorted_keys, void* bins, int bin_cap, int32_t* n_isects,
                        int32_t* flags, int long_min, const int32_t* order_ids, const int32_t* storage_of,
                        float* rows, void* stream);
int gsl_fused_clear_rows(float* rows, int N, void* stream);
int gsl_fused_raster_fwd(const float* Q0, const float* Q1, const float* Q2, int channels, int ed,
                         int width, int height, int tile_w, int tile_h, int ty0, int ty1,
                         const int32_t* tile_offsets, const int32_t* flatten_ids, int64_t capacity,
                         float* render, float* alphas, int32_t* last_ids, int row0, int row1, const void* Qh,
                         void* binned_ws, uint32_t* isect_hits, int32_t* isect_hit_counts, int long_min,
                         void* sort_bins, int bin_cap, int32_t* n_isects, int32_t* flags,
                         const int32_t* storage_of, void* stream);
/* sort_bins != NULL (binned projection, whole frame, bin_cap <= 2048, long_min == 0): every workgroup first does
 * gsl_fused_bin's work for its own tile -- adds up the sizes of the tiles before it, sorts its bin in LDS, writes
 * tile_offsets / flatten_ids (outputs then, despite the const) / n_isects and raises flags like gsl_fused_bin -- and
 * gsl_fused_bin is NOT called: the tracker's iteration goes without the sort launch.  The tile counters in binned_ws then
 * stay set until a compositing backward that is given clear_ws (gsl_fused_raster_bwd / gsl_tiny_raster_bwd) clears
 * them; after a forward nobody back-propagates the caller zeroes binned_ws before the next gsl_fused_project. */
int gsl_fused_raster_bwd(const float* Q0, const float* Q1, const float* Q2, int channels, int ed,
                         int width, int height, int tile_w, int tile_h, int ty0, int ty1,
                         const int32_t* tile_offsets, const int32_t* flatten_ids, int64_t capacity,
                         const float* render, const float* alphas, const int32_t* last_ids,
                         const float* v_render, const float* v_alphas, float* vacc, int row0, int row1,
                         const void* Qh, float* vrow, const uint32_t* isect_hits,
                         const int32_t* isect_hit_counts, int long_min, void* clear_ws, void* stream);
/* clear_ws (may be NULL): the binned_ws whose tile counters this backward clears (see gsl_fused_raster_fwd, sort_bins). */
/* Long tile lists split over workgroups (long_min > 0 in the calls above and in gsl_tiny_raster_bwd: tiles whose list
 * is longer than long_min entries are skipped there and handled here).  A pile of splats in one tile -- the invalid
 * pixels of a TUM depth frame, /root/reference/src/data/Image.py:29-35 -- is cut into segments of gsl_long_segment() entries, one
 * workgroup each: the forward computes per-pixel segment transmittances, restarts every segment from the product of
 * the earlier ones and combines the partial images; the backward restarts every segment from the stored state.
 * long_ws: gsl_long_ws_bytes(max_seg) bytes, zero-filled once; max_seg bounds the (tile, segment) pairs of a frame
 * (if a frame has more, long_ws[1] (int32) is set to the number needed: poll it, grow, re-run).  Call
 * gsl_long_raster_fwd after gsl_fused_raster_fwd, gsl_long_raster_bwd after gsl_fused_raster_bwd / gsl_tiny_raster_bwd
 * (it adds into vacc; gsl_fused_project_bwd given both tiny_trec and vacc consumes both). */
size_t gsl_long_ws_bytes(int max_seg);
int gsl_long_segment(void);      /* entries per compositing segment (callers size max_seg with it) */
int gsl_long_sort_segment(void); /* keys per sorted run of gsl_long_sort before its merge passes (sizes `passes`) */
/* Binned mode only: gsl_fused_bin(long_min > 0) leaves the lists longer than long_min unsorted, and gsl_long_sort (call it
 * right after) sorts them with one wave per gsl_long_sort_segment() keys (registers) + `passes` merge-path passes (2^passes such runs per
 * list at most; a longer list sets long_ws[2] (int32)), ping-ponging between sort_keys (scratch, packed) and the tile's
 * bin; flatten_ids receives the result.  One workgroup used to take 1.6 ms for a 23 k-entry list. */
int gsl_long_sort(const int32_t* tile_offsets, int tile_w, int tile_h, int ty0, int ty1, int64_t capacity,
                  uint64_t* bins, int bin_cap, uint64_t* sort_keys, int32_t* flatten_ids, int long_min,
                  void* long_ws, size_t long_ws_bytes, int max_seg, int passes, const int32_t* storage_of,
                  void* stream);
int gsl_long_raster_fwd(const float* Q0, const float* Q1, const float* Q2, int channels, int ed, int width,
                        int height, int tile_w, int tile_h, int ty0, int ty1, const int32_t* tile_offsets,
                        const int32_t* flatten_ids, int64_t capacity, float* render, float* alphas,
                        int32_t* last_ids, int row0, int row1, const void* Qh, uint32_t* isect_hits,
                        int long_min, void* long_ws, size_t long_ws_bytes, int max_seg, int map_ready, void* stream);
/* map_ready != 0: gsl_long_sort has already listed this frame's (tile, segment) pairs for the same strip, long_min and
 * max_seg in long_ws (binned mode); 0: list them here. */
int gsl_long_raster_bwd(const float* Q0, const float* Q1, const float* Q2, int channels, int ed, int width,
                        int height, int tile_w, int tile_h, int ty0, int ty1, const int32_t* tile_offsets,
                        const int32_t* flatten_ids, int64_t capacity, const float* render,
                        const float* alphas, const int32_t* last_ids, const float* v_render,
                        const float* v_alphas, float* vacc, int row0, int row1, const void* Qh,
                        const uint32_t* isect_hits, int long_min, void* long_ws, int max_seg, void* stream);
int gsl_fused_project_bwd(const float* means, const float* quats, const float* scales,
                          const float* opacities, const float* colors, int sh_degree, int K_sh,
                          const float* viewmat, const float* K, int N, int width, int height,
                          float eps2d, int antialiased, int channels, const int32_t* radii,
                          const float* Q1, const float* compensations, float* vacc, float* v_means,
                          float* v_quats, float* v_scales, float* v_opacities, float* v_colors,
                          float* v_viewmat, void* ws, size_t ws_bytes, int n_tiles, const float* vrow,
                          const uint64_t* sorted_keys, const int32_t* tile_offsets, const float* Q0, int tile_w,
                          int tile_h, int ty0, int ty1, int64_t capacity, float* tiny_trec, const float* tiny_vcT,
                          int reduce_viewmat, int32_t* v_colors_state, void* stream);
int gsl_fused_project_bwd_keep(const float* means, const float* quats, const float* scales,
                               const float* opacities, const float* colors, int sh_degree, int K_sh,
                               const float* viewmat, const float* K, int N, int width, int height,
                               float eps2d, int antialiased, int channels, const int32_t* radii,
                               const float* Q1, const float* compensations, float* vacc, float* v_means,
                               float* v_quats, float* v_scales, float* v_opacities, float* v_colors,
                               float* v_viewmat, void* ws, size_t ws_bytes, int n_tiles, const float* vrow,
                               const uint64_t* sorted_keys, const int32_t* tile_offsets, const float* Q0, int tile_w,
                               int tile_h, int ty0, int ty1, int64_t capacity, float* tiny_trec, const float* tiny_vcT,
                               int reduce_viewmat, int32_t* v_colors_state, void* stream);
/* v_colors_state (int32[1], may be NULL): the caller's promise that v_colors is the SAME buffer in every call that is
 * given this state word; initialise it to 1 together with a zero-filled v_colors (or to 0 for a buffer of unknown
 * content).  While it reads 1 a Gaussian whose colour gradient is zero -- all of them under a depth-only loss,
 * /root/reference/src/my_gsplat/gs_trainer_total.py:111-123 -- skips its zero stores (48 of the ~92 bytes per Gaussian the
 * call writes at SH degree 1); a launch that writes a real colour gradient marks the buffer dirty and the following
 * launch stores everything again.  Maintained by the reduction kernel (reduce_viewmat = 1). */
const float* gsl_fused_viewmat_rows(const void* ws, int n_tiles);

/* "Tiny splat" backward: valid when every r_cull (Q1[:,3]) is < 2 px, i.e. no splat reaches more than 4x4
 * pixel centres (GsplatLoc's as-coded scales).  gsl_tiny_raster_bwd replaces gsl_fused_raster_bwd: instead of
 * reducing and accumulating gradient rows it stores per (splat, pixel) records into trec[N][16][2] (zero on
 * entry) and the chained upstream gradient of every pixel into vcT[H,W,channels]; gsl_fused_project_bwd given
 * tiny_trec / tiny_vcT then sums each Gaussian's 4x4 slab into its gradient row (in LDS, four lanes per Gaussian)
 * and clears the slab.  flags (int32[1], may be NULL): flags[0] is set to 1 when a
 * (pixel, splat) pair fell outside its slab, i.e. the precondition did not hold and the gradients are
 * incomplete -- the caller polls it and re-runs the iteration with gsl_fused_raster_bwd. */
int gsl_tiny_raster_bwd(const float* Q0, const float* Q1, const float* Q2, int channels, int ed,
                        int width, int height, int tile_w, int tile_h, int ty0, int ty1,
                        const int32_t* tile_offsets, const int32_t* flatten_ids, int64_t capacity,
                        const float* render, const float* alphas, const int32_t* last_ids,
                        const float* v_render, const float* v_alphas, float* trec, float* vcT,
                        int row0, int row1, int32_t* flags, int long_min, const float* loss_depth_gt,
                        float depth_lambda, float edge_lambda, float* loss_partials, void* clear_ws, void* stream);
/* loss_depth_gt != NULL (whole frame, channels 1 or 4): the kernel computes the tracking loss of gsl_tracking_loss for
 * its tile itself -- the tile is that kernel's 16x16 block -- WRITES v_render's depth channel and
 * loss_partials[tiles][2], and back-propagates from that gradient (v_render's other channels count as zero): the
 * tracker's iteration then goes without the separate loss launch.  NULL: v_render is read as given. */

/* ---- tracker tail: loss + pose update on device (csrc/tracker.hip) ----
 * Replaces the PyTorch/kornia glue of one iteration of GsplatLoc's Runner.train
 * (/root/reference/src/my_gsplat/gs_trainer_total.py:105-185,265-267; loss.py:10-59; model.py:79-116).
 *
 * gsl_tracking_loss: depth L1 + Sobel-edge L1 of render[...,channels-1] against depth_gt[H,W] over the owned
 *   pixel rows [row0,row1) (whole image: 0,height), normalised by width*height; writes d loss / d depth into
 *   v_render[...,channels-1] for rows [row0-1,row1+1) and the block sums (sum|a-b|, sum|Sa-Sb|) into
 *   loss_partials[gsl_loss_n_partials(width,height,row0,row1)][2] (inside ws when NULL; ws may be NULL otherwise).
 *   One launch: 16x16 pixel blocks with a two-pixel apron through LDS.  ws: gsl_loss_ws_bytes.
 * gsl_pose_init : pose state <- init_c2w (wxyz quaternion + translation), zero Adam moments, step 0; writes
 *   c2w[16] and viewmat[16] = c2w^-1.  pose_f[40] floats, pose_i[4] ints (layout: csrc/tracker.hip).
 * gsl_pose_step : finish the loss, pose errors vs gt_c2w, early-stop bookkeeping (best loss after min_step,
 *   patience), pose chain viewmat->(quat,t), two Adam updates (weight decay in the gradient), lr = lr0 gamma^step,
 *   new c2w / viewmat; appends the loss to loss_hist[max_steps] (may be NULL).  Does nothing once stopped
 *   (pose_i[2]); c2w / viewmat then hold the last pose that was rendered (the iteration that reaches max_steps takes
 *   its Adam step but leaves them).  beta1, beta2 and gamma are doubles, as torch.optim keeps them: 1 - beta, the
 *   bias corrections and gamma^step are taken in double and rounded once.  The pose gradient is v_viewmat[16], or -- vm_rows not NULL -- the n_vm_rows partial rows a
 *   gsl_fused_project_bwd(reduce_viewmat = 0) left (K and the viewmat buffer, which still holds the rendered pose, are
 *   read for the camera-position chain).  loss_sums[3] (already summed over ranks: the two sums and the row-cosine
 *   sum) overrides loss_partials / normal_sum when not NULL.  normal_lambda != 0 adds normal_lambda * (1 - normal_sum / (3 height)).
 * gsl_normal_loss: the normal-consistency term the reference defines and keeps switched off (loss.py:62-101 "cosine",
 *   geometry.py:164-197; call commented out at gs_trainer_total.py:138-143, normal_lambda = 0 at data/base.py:28):
 *   unit normals of the back-projected masked depth images (central differences, replicated borders), cosine
 *   similarity ALONG EACH IMAGE ROW per component as the reference codes it, loss = 1 - mean.  Adds
 *   normal_lambda * d loss / d depth to v_render[...,channels-1] for rows [row0-1,row1+1) (call it after
 *   gsl_tracking_loss, which writes that channel) and writes the sum of the owned rows' cosines to normal_sum[0].
 *   ws: gsl_normal_ws_bytes.
 * gsl_photo_loss: the photometric term the reference declares and keeps commented out (gs_trainer_total.py:111-123,
 *   ssim_lambda = 0.5 at data/base.py:26, StructuralSimilarityIndexMeasure(data_range=1.0)) (csrc/photo.hip).  With
 *   m = (render[...,3] != 0) (no gradient), c = render[...,0:3] m and p = pixels m (pixels [H,W,3] in 0..1):
 *     l1 = sum |c - p| / (sum m + 1e-8)  (sum m counts pixels),  ssim = mean of S over the 3 (H-10) (W-10) windows
 *     inside the image, S as torchmetrics computes it for data_range 1 (11x11 window of a sigma 1.5 Gaussian, C1 = 1e-4,
 *     C2 = 9e-4, variances clamped at 0),  photo = (1 - ssim_lambda) l1 + ssim_lambda (1 - ssim).
 *   WRITES rgb_lambda * d photo / d render into v_render[...,0:3] of every pixel (exactly 0 where m = 0), leaves
 *   v_render[...,3] untouched (so it composes with gsl_tracking_loss / gsl_normal_loss in either order) and writes the
 *   raw sums photo_sums[3] = (sum m, sum |c - p|, sum S).  Whole frame only (a strip would need a 5-row halo), channels
 *   must be 4 and both sides at least 11 (GSL_ERR_BAD_ARG otherwise).  Two launches, no atomics: two calls give the
 *   same bits.  ws: gsl_photo_ws_bytes (0 for a frame below 11x11); GSL_ERR_WORKSPACE when shorter.
 * gsl_pose_step_photo: gsl_pose_step with the photometric term: photo_sums (of gsl_photo_loss; NULL: none) adds
 *   rgb_lambda * photo, taken in double from the three sums, to the total that goes into loss_hist, the best-loss
 *   bookkeeping and the early stop; whenever pose_f[23] is written, pose_f[34] gets that step's l1 and pose_f[35] its
 *   1 - ssim.  gsl_pose_step is this function with NULL, 0, 0.
 * gsl_pose_step_best: gsl_pose_step_photo (photo_sums may be NULL: no photometric term) that also keeps the
 *   minimum-loss POSE: whenever pose_f[23] is written, best_pose[24] (not NULL: GSL_ERR_BAD_ARG) gets the pose that
 *   iteration rendered with, i.e. before its Adam update --
 *     best_pose[0..3] the quaternion as stored (wxyz, not normalised), [4..6] the translation, [7] the total loss
 *     (== pose_f[23]), [8..23] the 4x4 camera-to-world matrix, the bits c2w held during that iteration.
 *   Nothing else is written to it: "no best yet" is pose_i[3] == -1, and the buffer then holds what the caller left.
 *   Every other output is bit-identical to gsl_pose_step_photo's. */
size_t gsl_photo_ws_bytes(int width, int height);
int gsl_photo_loss(const float* render, int channels, const float* pixels, int width, int height, float rgb_lambda,
                   float ssim_lambda, float* v_render, float* photo_sums, void* ws, size_t ws_bytes, void* stream);
int gsl_pose_step_photo(float* pose_f, int* pose_i, const float* v_viewmat, const float* vm_rows, int n_vm_rows,
                        const float* K, const float* loss_partials, int n_partials, const float* loss_sums,
                        const float* normal_sum, const float* gt_c2w, int width, int height, float depth_lambda,
                        float edge_lambda, float normal_lambda, double beta1, double beta2, float eps, float wd_quat,
                        float wd_trans, double gamma, int min_step, int patience, int early_stop, int max_steps,
                        float* c2w, float* viewmat, float* loss_hist, void* stream, const float* photo_sums,
                        float rgb_lambda, float ssim_lambda);
int gsl_pose_step_best(float* pose_f, int* pose_i, const float* v_viewmat, const float* vm_rows, int n_vm_rows,
                       const float* K, const float* loss_partials, int n_partials, const float* loss_sums,
                       const float* normal_sum, const float* gt_c2w, int width, int height, float depth_lambda,
                       float edge_lambda, float normal_lambda, double beta1, double beta2, float eps, float wd_quat,
                       float wd_trans, double gamma, int min_step, int patience, int early_stop, int max_steps,
                       float* c2w, float* viewmat, float* loss_hist, void* stream, const float* photo_sums,
                       float rgb_lambda, float ssim_lambda, float* best_pose);
size_t gsl_loss_ws_bytes(int width, int height);
int gsl_loss_n_partials(int width, int height, int row0, int row1);
size_t gsl_normal_ws_bytes(int width, int height);
int gsl_normal_loss(const float* render, int channels, const float* depth_gt, int width, int height, int row0,
                    int row1, float fx, float fy, float cx, float cy, float normal_lambda, float* v_render,
                    float* normal_sum, void* ws, size_t ws_bytes, void* stream);
int gsl_tracking_loss(const float* render, int channels, const float* depth_gt, int width, int height,
                      int row0, int row1, float depth_lambda, float edge_lambda, float* v_render,
                      float* loss_partials, int* n_partials_host, void* ws, size_t ws_bytes, void* stream);
int gsl_pose_init(float* pose_f, int* pose_i, const float* init_c2w, float lr_quat, float lr_trans,
                  float* c2w, float* viewmat, void* stream);
int gsl_pose_step(float* pose_f, int* pose_i, const float* v_viewmat, const float* vm_rows, int n_vm_rows,
                  const float* K, const float* loss_partials, int n_partials, const float* loss_sums, const float* normal_sum, const float* gt_c2w,
                  int width, int height, float depth_lambda, float edge_lambda, float normal_lambda,
                  double beta1, double beta2, float eps,
                  float wd_quat, float wd_trans, double gamma, int min_step, int patience, int early_stop,
                  int max_steps, float* c2w, float* viewmat, float* loss_hist, void* stream);
/* Several GPUs: what one rank contributes to the ONE all-reduce of an iteration.  out16[0..11] =
 * v_viewmat[0..11] of its strip (given reduced, or as vm_rows with the viewmat and K they were computed at), out16[12..13] = its (sum |d - g|, sum |S(d) - S(g)|) over loss_partials[n][2]
 * (fixed order), out16[14] = normal_sum[0] (0 when NULL), out16[15] = 0.  After the all-reduce (sum) gsl_pose_step
 * takes v_viewmat = out16 and loss_sums = out16 + 12.  Written by a kernel of this library so that a captured
 * iteration holds no foreign node. */
int gsl_pack_pose_reduce(const float* v_viewmat, const float* vm_rows, int n_vm_rows, const float* viewmat,
                         const float* K, const float* loss_partials, int n_partials, const float* normal_sum,
                         float* out16, void* stream);

/* ---- per-frame set-up: exact k nearest neighbours on the device (csrc/knn.hip) ----
 * Stands in for the small_gicp KdTree search of /root/reference/src/my_gsplat/utils.py:16-22.
 * points[N,3]; bbox[6] = (min x,y,z, max x,y,z) on the device; uniform grid of gsl_knn_cells() cells.
 * gsl_knn_count fills the per-cell counts at the start of ws (int32[cells]); the caller turns them into an
 * inclusive cumulative sum incl_offsets[cells] (any device scan); gsl_knn_query then writes the SQUARED
 * distances to the k <= 8 nearest points (the point itself included), ascending, into dists[N,k].  A cloud of
 * N < k points has only N neighbours per query: the remaining slots hold +inf (as a KD-tree query reports them). */
size_t gsl_knn_ws_bytes(int N);
int gsl_knn_cells(void);
int gsl_knn_count(const float* points, int N, const float* bbox, void* ws, size_t ws_bytes, void* stream);
int gsl_knn_query(const float* points, int N, const float* bbox, const int32_t* incl_offsets, int k,
                  float* dists, void* ws, size_t ws_bytes, void* stream);

/* ---- absolute screen-space gradient: gsplat's means2d.absgrad (rasterization(absgrad=True)) (csrc/absgrad.hip) ----
 * For every Gaussian, sum over pixels p of |dL_p / d means2d| per component (x, y), L_p = <v_render_p, render_p> +
 * v_alpha_p alpha_p: the per-pixel terms whose plain sum is the v_means2d of the compositing backward.  Both entries
 * ACCUMULATE into absgrad[n][2], zeroed by the caller, rows indexed like flatten_ids.  Whole frame only, 16x16 tiles.
 * gsl_fused_absgrad: the records, lists and outputs of gsl_fused_project / _bin / _raster_fwd (no long-list segments,
 *   float32 records), channels 1 / 3 / 4, ed as there; render is read for ed only.  isect_hits / isect_hit_counts
 *   (may be NULL together): the forward's hit lists -- each quadrant then walks only the entries it composited.
 * gsl_rasterize_absgrad: the arrays of gsl_rasterize_fwd / _bwd for one camera (same channel counts, backgrounds may
 *   be NULL); call once per camera with its tile_offsets, as gsl_rasterize_bwd; t_final (may be NULL) as there. */
int gsl_fused_absgrad(const float* Q0, const float* Q1, const float* Q2, int channels, int ed, int width, int height,
                      int tile_w, int tile_h, const int32_t* tile_offsets, const int32_t* flatten_ids, int64_t capacity,
                      const float* render, const float* alphas, const int32_t* last_ids, const float* v_render,
                      const float* v_alphas, const uint32_t* isect_hits, const int32_t* isect_hit_counts,
                      float* absgrad, void* stream);
int gsl_rasterize_absgrad(const float* means2d, const float* conics, const float* colors, const float* opacities,
                          const float* backgrounds, int channels, int width, int height, int tile_size, int tile_w,
                          int tile_h, const int32_t* tile_offsets, const int32_t* flatten_ids, int64_t capacity,
                          const float* render_alphas, const int32_t* last_ids, const float* t_final,
                          const float* v_render_colors, const float* v_render_alphas, float* absgrad, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* GSLOC_HIP_H */
