"""One Python caller per C entry point of the fused pipeline (include/gsloc_hip.h).

Each carries the header's parameter names in the header's order, takes tensors, sizes a workspace from its tensor and
launches on torch's current stream.  What the header documents as NULL / 0 for a mode that is off (fp16 staging, bins,
deterministic rows, hit lists, long lists, placement, tiny slabs, the fused loss) is keyword-only and defaults to off.
What the header never lets be NULL is read with ``.data_ptr()`` directly, the rest through ``ptr()``: a call per argument
adds up on the eager drop-in path.  No other module calls these; tests/test_stages_cpu.py and
tests/test_rows_cleared_by_sort_cpu.py pin them to the header.
"""
from __future__ import annotations

import math

import torch

from ._lib import check, current_stream, load_library, ptr

MAX_STRIP_TILES = 8192
_MODES = {"RGB": (3, False), "D": (1, False), "ED": (1, True), "RGB+D": (4, False), "RGB+ED": (4, True)}


def tile_n_bits(n_tiles: int) -> int:
    return int(math.floor(math.log2(n_tiles))) + 1


def alloc_records(N: int, rgb: bool, dev, zero: bool = False):
    """The per-Gaussian record arrays Q0, Q1, Q2 ([N,4] each; Q2 None without colours)."""
    make = torch.zeros if zero else torch.empty
    Q0, Q1 = (make(N, 4, dtype=torch.float32, device=dev) for _ in range(2))
    Q2 = make(N, 4, dtype=torch.float32, device=dev) if rgb else None
    return Q0, Q1, Q2


def fused_project(means, quats, scales, opacities, colors, sh_degree, K_sh, viewmat, K, N, width, height, eps2d, near_plane,
                  far_plane, radius_clip, antialiased, tile_w, tile_h, ty0, ty1, radii, Q0, Q1, Q2, compensations,
                  tiles_per_gauss, tile_offsets, n_isects, ws, *, Qh=None, bins=None, bin_cap=0, flags=None, order_ids=None):
    check(load_library().gsl_fused_project(
        means.data_ptr(), quats.data_ptr(), scales.data_ptr(), opacities.data_ptr(), ptr(colors), sh_degree, K_sh,
        viewmat.data_ptr(), K.data_ptr(), N, width, height, eps2d, near_plane, far_plane, radius_clip, antialiased, tile_w,
        tile_h, ty0, ty1, radii.data_ptr(), Q0.data_ptr(), Q1.data_ptr(), ptr(Q2), ptr(compensations), ptr(tiles_per_gauss),
        tile_offsets.data_ptr(), n_isects.data_ptr(), ws.data_ptr(), ws.numel(), ptr(Qh), ptr(bins), bin_cap, ptr(flags),
        ptr(order_ids), current_stream()), "gsl_fused_project")


def fused_bin(Q0, radii, N, tile_w, tile_h, ty0, ty1, tile_n_bits, tile_offsets, capacity, sort_keys, flatten_ids, ws, *,
              isect_ids=None, write_sorted_keys=0, bins=None, bin_cap=0, n_isects=None, flags=None, long_min=0,
              order_ids=None, storage_of=None):
    check(load_library().gsl_fused_bin(
        Q0.data_ptr(), radii.data_ptr(), N, tile_w, tile_h, ty0, ty1, tile_n_bits, tile_offsets.data_ptr(), capacity,
        sort_keys.data_ptr(), ptr(flatten_ids), ptr(isect_ids), ws.data_ptr(), ws.numel(), write_sorted_keys, ptr(bins),
        bin_cap, ptr(n_isects), ptr(flags), long_min, ptr(order_ids), ptr(storage_of), current_stream()), "gsl_fused_bin")


def fused_bin_clear(Q0, radii, N, tile_w, tile_h, ty0, ty1, tile_n_bits, tile_offsets, capacity, sort_keys, flatten_ids, ws,
                    rows, *, isect_ids=None, write_sorted_keys=0, bins=None, bin_cap=0, n_isects=None, flags=None,
                    long_min=0, order_ids=None, storage_of=None):
    """fused_bin whose sort launch also zeroes the N gradient rows."""
    check(load_library().gsl_fused_bin_clear(
        Q0.data_ptr(), radii.data_ptr(), N, tile_w, tile_h, ty0, ty1, tile_n_bits, tile_offsets.data_ptr(), capacity,
        sort_keys.data_ptr(), ptr(flatten_ids), ptr(isect_ids), ws.data_ptr(), ws.numel(), write_sorted_keys, ptr(bins),
        bin_cap, ptr(n_isects), ptr(flags), long_min, ptr(order_ids), ptr(storage_of), ptr(rows), current_stream()),
        "gsl_fused_bin_clear")


def fused_clear_rows(rows, N):
    check(load_library().gsl_fused_clear_rows(ptr(rows), N, current_stream()), "gsl_fused_clear_rows")


def fused_raster_fwd(Q0, Q1, Q2, channels, ed, width, height, tile_w, tile_h, ty0, ty1, tile_offsets, flatten_ids, capacity,
                     render, alphas, last_ids, row0, row1, *, Qh=None, binned_ws=None, isect_hits=None, isect_hit_counts=None,
                     long_min=0, sort_bins=None, bin_cap=0, n_isects=None, flags=None, storage_of=None):
    check(load_library().gsl_fused_raster_fwd(
        ptr(Q0), ptr(Q1), ptr(Q2), channels, ed, width, height, tile_w, tile_h, ty0, ty1, tile_offsets.data_ptr(),
        ptr(flatten_ids), capacity, render.data_ptr(), alphas.data_ptr(), last_ids.data_ptr(), row0, row1, ptr(Qh),
        ptr(binned_ws), ptr(isect_hits), ptr(isect_hit_counts), long_min, ptr(sort_bins), bin_cap, ptr(n_isects), ptr(flags),
        ptr(storage_of), current_stream()), "gsl_fused_raster_fwd")


def fused_raster_bwd(Q0, Q1, Q2, channels, ed, width, height, tile_w, tile_h, ty0, ty1, tile_offsets, flatten_ids, capacity,
                     render, alphas, last_ids, v_render, v_alphas, vacc, row0, row1, *, Qh=None, vrow=None, isect_hits=None,
                     isect_hit_counts=None, long_min=0, clear_ws=None):
    check(load_library().gsl_fused_raster_bwd(
        ptr(Q0), ptr(Q1), ptr(Q2), channels, ed, width, height, tile_w, tile_h, ty0, ty1, tile_offsets.data_ptr(),
        ptr(flatten_ids), capacity, render.data_ptr(), alphas.data_ptr(), last_ids.data_ptr(), v_render.data_ptr(),
        v_alphas.data_ptr(), ptr(vacc), row0, row1, ptr(Qh), ptr(vrow), ptr(isect_hits), ptr(isect_hit_counts), long_min,
        ptr(clear_ws), current_stream()), "gsl_fused_raster_bwd")


def tiny_raster_bwd(Q0, Q1, Q2, channels, ed, width, height, tile_w, tile_h, ty0, ty1, tile_offsets, flatten_ids, capacity,
                    render, alphas, last_ids, v_render, v_alphas, trec, vcT, row0, row1, *, flags=None, long_min=0,
                    loss_depth_gt=None, depth_lambda=0.0, edge_lambda=0.0, loss_partials=None, clear_ws=None):
    check(load_library().gsl_tiny_raster_bwd(
        ptr(Q0), ptr(Q1), ptr(Q2), channels, ed, width, height, tile_w, tile_h, ty0, ty1, tile_offsets.data_ptr(),
        ptr(flatten_ids), capacity, render.data_ptr(), alphas.data_ptr(), last_ids.data_ptr(), v_render.data_ptr(),
        v_alphas.data_ptr(), trec.data_ptr(), vcT.data_ptr(), row0, row1, ptr(flags), long_min, ptr(loss_depth_gt),
        depth_lambda, edge_lambda, ptr(loss_partials), ptr(clear_ws), current_stream()), "gsl_tiny_raster_bwd")


def long_sort(tile_offsets, tile_w, tile_h, ty0, ty1, capacity, bins, bin_cap, sort_keys, flatten_ids, long_min, long_ws,
              max_seg, passes, *, storage_of=None):
    check(load_library().gsl_long_sort(
        tile_offsets.data_ptr(), tile_w, tile_h, ty0, ty1, capacity, bins.data_ptr(), bin_cap, sort_keys.data_ptr(),
        flatten_ids.data_ptr(), long_min, long_ws.data_ptr(), long_ws.numel(), max_seg, passes, ptr(storage_of),
        current_stream()), "gsl_long_sort")


def long_raster_fwd(Q0, Q1, Q2, channels, ed, width, height, tile_w, tile_h, ty0, ty1, tile_offsets, flatten_ids, capacity,
                    render, alphas, last_ids, row0, row1, long_min, long_ws, max_seg, map_ready, *, Qh=None, isect_hits=None):
    check(load_library().gsl_long_raster_fwd(
        ptr(Q0), ptr(Q1), ptr(Q2), channels, ed, width, height, tile_w, tile_h, ty0, ty1, tile_offsets.data_ptr(),
        flatten_ids.data_ptr(), capacity, render.data_ptr(), alphas.data_ptr(), last_ids.data_ptr(), row0, row1, ptr(Qh),
        ptr(isect_hits), long_min, long_ws.data_ptr(), long_ws.numel(), max_seg, map_ready, current_stream()),
        "gsl_long_raster_fwd")


def long_raster_bwd(Q0, Q1, Q2, channels, ed, width, height, tile_w, tile_h, ty0, ty1, tile_offsets, flatten_ids, capacity,
                    render, alphas, last_ids, v_render, v_alphas, vacc, row0, row1, long_min, long_ws, max_seg, *, Qh=None,
                    isect_hits=None):
    check(load_library().gsl_long_raster_bwd(
        ptr(Q0), ptr(Q1), ptr(Q2), channels, ed, width, height, tile_w, tile_h, ty0, ty1, tile_offsets.data_ptr(),
        flatten_ids.data_ptr(), capacity, render.data_ptr(), alphas.data_ptr(), last_ids.data_ptr(), v_render.data_ptr(),
        v_alphas.data_ptr(), vacc.data_ptr(), row0, row1, ptr(Qh), ptr(isect_hits), long_min, long_ws.data_ptr(), max_seg,
        current_stream()), "gsl_long_raster_bwd")


def fused_project_bwd(means, quats, scales, opacities, colors, sh_degree, K_sh, viewmat, K, N, width, height, eps2d,
                      antialiased, channels, radii, Q1, compensations, vacc, v_means, v_quats, v_scales, v_opacities,
                      v_colors, v_viewmat, ws, n_tiles, reduce_viewmat, *, vrow=None, sorted_keys=None, tile_offsets=None,
                      Q0=None, tile_w=0, tile_h=0, ty0=0, ty1=0, capacity=0, tiny_trec=None, tiny_vcT=None,
                      v_colors_state=None):
    check(load_library().gsl_fused_project_bwd(
        means.data_ptr(), quats.data_ptr(), scales.data_ptr(), opacities.data_ptr(), ptr(colors), sh_degree, K_sh,
        viewmat.data_ptr(), K.data_ptr(), N, width, height, eps2d, antialiased, channels, radii.data_ptr(), Q1.data_ptr(),
        ptr(compensations), ptr(vacc), ptr(v_means), ptr(v_quats), ptr(v_scales), ptr(v_opacities), ptr(v_colors),
        ptr(v_viewmat), ws.data_ptr(), ws.numel(), n_tiles, ptr(vrow), ptr(sorted_keys), ptr(tile_offsets), ptr(Q0), tile_w,
        tile_h, ty0, ty1, capacity, ptr(tiny_trec), ptr(tiny_vcT), reduce_viewmat, ptr(v_colors_state), current_stream()),
        "gsl_fused_project_bwd")


def fused_project_bwd_keep(means, quats, scales, opacities, colors, sh_degree, K_sh, viewmat, K, N, width, height, eps2d,
                           antialiased, channels, radii, Q1, compensations, vacc, v_means, v_quats, v_scales, v_opacities,
                           v_colors, v_viewmat, ws, n_tiles, reduce_viewmat, *, vrow=None, sorted_keys=None,
                           tile_offsets=None, Q0=None, tile_w=0, tile_h=0, ty0=0, ty1=0, capacity=0, tiny_trec=None,
                           tiny_vcT=None, v_colors_state=None):
    """fused_project_bwd (general path) that reads the gradient rows and leaves them standing."""
    check(load_library().gsl_fused_project_bwd_keep(
        means.data_ptr(), quats.data_ptr(), scales.data_ptr(), opacities.data_ptr(), ptr(colors), sh_degree, K_sh,
        viewmat.data_ptr(), K.data_ptr(), N, width, height, eps2d, antialiased, channels, radii.data_ptr(), Q1.data_ptr(),
        ptr(compensations), ptr(vacc), ptr(v_means), ptr(v_quats), ptr(v_scales), ptr(v_opacities), ptr(v_colors),
        ptr(v_viewmat), ws.data_ptr(), ws.numel(), n_tiles, ptr(vrow), ptr(sorted_keys), ptr(tile_offsets), ptr(Q0), tile_w,
        tile_h, ty0, ty1, capacity, ptr(tiny_trec), ptr(tiny_vcT), reduce_viewmat, ptr(v_colors_state), current_stream()),
        "gsl_fused_project_bwd_keep")


def fused_absgrad(Q0, Q1, Q2, channels, ed, width, height, tile_w, tile_h, tile_offsets, flatten_ids, capacity, render,
                  alphas, last_ids, v_render, v_alphas, absgrad, *, isect_hits=None, isect_hit_counts=None):
    check(load_library().gsl_fused_absgrad(
        ptr(Q0), ptr(Q1), ptr(Q2), channels, ed, width, height, tile_w, tile_h, tile_offsets.data_ptr(), ptr(flatten_ids),
        capacity, render.data_ptr(), alphas.data_ptr(), last_ids.data_ptr(), v_render.data_ptr(), v_alphas.data_ptr(),
        ptr(isect_hits), ptr(isect_hit_counts), absgrad.data_ptr(), current_stream()), "gsl_fused_absgrad")
