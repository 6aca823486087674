"""Sequence evaluation driver -- the role of /root/reference/src/GsplatLoc_eval.py + Runner.train +
eval/logger.py:258-304 without W&B: track every consecutive frame pair of a room from the ground-truth pose
of frame i, record the error of the minimum-loss iterate against frame i+1, and report
ATE := RMSE of the translation errors, AAE := RMSE of the rotation errors (eval/utils.py:113-119), in the
res.json layout of /root/reference/docs/res.json.

    python -m gsplatloc_amd.eval --dataset Replica --rooms room0 --root /data/Replica --num-iters 200

--sequential: the room is tracked from the ground-truth pose of frame 0 ONLY (gsplatloc_amd.localizer.Localizer): every
later frame is placed with, and started from, the tracker's own estimates, and the errors reported are the ABSOLUTE
errors of the estimated trajectory against ground truth (no trajectory alignment), i.e. they include the drift.
"""
from __future__ import annotations

import argparse
import json
import math
import time
from typing import Dict, List, Optional

import torch

from .data import Parser
from .graph_tracker import GraphTracker
from .localizer import Localizer
from .mapping import MapConfig
from .my_gsplat import TrackerConfig, init_gs_scales


def rmse(values: List[float]) -> float:
    """eval/utils.py:113-119."""
    return math.sqrt(sum(v * v for v in values) / max(len(values), 1))


def evaluate_room(parser: Parser, num_iters: int = 2000, max_frames: Optional[int] = 1998, verbose: bool = False,
                  profile: bool = False, rgb_lambda: float = 0.0, ssim_lambda: float = 0.5, sequential: bool = False,
                  motion: str = "constant_velocity", map_mode: bool = False,
                  map_capacity: Optional[int] = None, map_view_guard: Optional[float] = None,
                  map_free_rho: Optional[float] = None, map_free_window: int = 1, map_evict: bool = False,
                  map_merge_voxel: Optional[float] = None, map_merge_every: int = 1, map_reloc: bool = False,
                  map_reloc_min_agree: Optional[float] = None, map_reloc_rot_deg: Optional[float] = None,
                  map_reloc_trans: Optional[float] = None, map_keyframes: bool = False,
                  map_keyframe_rot_deg: Optional[float] = None, map_keyframe_trans: Optional[float] = None,
                  map_refine: bool = False, map_refine_max_weight: Optional[int] = None,
                  map_info: bool = False, map_align: bool = False, map_align_steps: Optional[int] = None,
                  map_origins: bool = False, map_loop: bool = False, map_loop_min_gap: Optional[int] = None,
                  map_align_accept: bool = False, map_reloc_align_top: Optional[int] = None,
                  map_view_occlusion: Optional[float] = None, map_view_occlusion_cell: Optional[int] = None,
                  map_view_occlusion_window: Optional[int] = None, map_photo_scale: Optional[float] = None,
                  map_photo_max_residual: Optional[float] = None, map_align_levels: Optional[int] = None,
                  map_align_level_steps: Optional[int] = None, map_photo_exposure: bool = False) -> Dict:
    """Runner.train (gs_trainer_total.py:45-282): frames 0..min(len, 1998).  profile=True: also the wall time per phase
    of a frame (synchronising at the phase boundaries): reading + back-projection + PCA normalisation, the query-depth
    render, the kNN scale initialisation, load_frame (copies + calibration pass), and the optimisation itself (graph
    capture + replays + polls) -- `phase_seconds` in the result.  rgb_lambda != 0 switches the photometric term on
    (TrackerConfig.rgb_lambda / ssim_lambda): the tracker then renders "RGB+ED" and is given the frame's image.
    sequential=True: evaluate_sequential (only frame 0's ground-truth pose is used; ``motion`` is its hand-over;
    ``map_mode``: frames are tracked against a map grown on the device, of ``map_capacity`` rows at most;
    ``map_view_guard``: against the part of it in view, the image widened by that many pixels; ``map_free_rho`` /
    ``map_free_window``: MapConfig.free_rho / free_window_px, the rows a frame sees through are removed;
    ``map_evict``: MapConfig.evict, a frame that does not fit evicts the least recently observed rows;
    ``map_merge_voxel`` / ``map_merge_every``: MapConfig.merge_voxel / merge_every, the rows that share a voxel of that
    side are fused after every that-many-th frame; ``map_reloc``: MapConfig.reloc, an estimate the map does not confirm
    is tracked once more from the best-scoring pose of a grid around the start poses, with ``map_reloc_min_agree`` /
    ``map_reloc_rot_deg`` / ``map_reloc_trans`` for MapConfig.reloc_min_agree / reloc_rot_deg / reloc_trans where not
    None; ``map_keyframes``: MapConfig.keyframes, a frame that stays lost is compared with the keyframes of the map and
    tracked once more from the best-scoring pose around the most similar ones, with ``map_keyframe_rot_deg`` /
    ``map_keyframe_trans`` for MapConfig.keyframe_rot_deg / keyframe_trans where not None; ``map_refine``:
    MapConfig.refine, the rows a frame observes again move to the running mean of their depths, with
    ``map_refine_max_weight`` for MapConfig.refine_max_weight where not None; ``map_info``: MapConfig.info, every frame
    that is not lost reports the covariance of its pose from the map's rows against its depth image; ``map_align``:
    MapConfig.align, every frame's start pose is aligned to the map by Gauss-Newton steps before the tracker runs, with
    ``map_align_steps`` for MapConfig.align_steps where not None; ``map_align_accept``: MapConfig.align_accept, a
    converged alignment that the map's rows pin down is the frame's pose and the tracker does not run;
    ``map_reloc_align_top``: MapConfig.reloc_align_top, that many of the best relocalisation candidates are aligned to
    the map before the winner is chosen; ``map_view_occlusion``: MapConfig.view_occlusion_rho, the rows of the guarded
    view that nearer rows of the map hide are not tracked, with ``map_view_occlusion_cell`` /
    ``map_view_occlusion_window`` for MapConfig.view_occlusion_cell_px / view_occlusion_window where not None;
    ``map_photo_scale``: MapConfig.photo_scale, the normal equations of map_info, map_align and map_loop gain a
    photometric term from the rows' colours against the frame's image, with ``map_photo_max_residual`` for
    MapConfig.photo_max_residual where not None, and ``map_photo_exposure`` for MapConfig.photo_exposure (every frame's
    gain and offset are estimated against the map and its image corrected; the report gains exposure_per_frame); ``map_align_levels``: MapConfig.align_levels, the alignments of
    map_align and map_loop run coarse to fine on an image pyramid of the frame, with ``map_align_level_steps`` for
    MapConfig.align_level_steps where not None)."""
    cfg = TrackerConfig(max_steps=num_iters, rgb_lambda=rgb_lambda, ssim_lambda=ssim_lambda)
    occlusion = {k: v for k, v in (("view_occlusion_cell_px", map_view_occlusion_cell),
                                   ("view_occlusion_window", map_view_occlusion_window)) if v is not None}
    if (map_view_occlusion is not None or occlusion) and map_view_guard is None:
        raise ValueError("map_view_occlusion belongs to the guarded view (map_view_guard)")
    if occlusion and map_view_occlusion is None:
        raise ValueError(f"{', '.join('map_' + k for k in occlusion)}: options of map_view_occlusion")
    if map_view_occlusion is not None:
        occlusion["view_occlusion_rho"] = map_view_occlusion
    if map_merge_voxel is not None and not map_mode:
        raise ValueError("map_merge_voxel belongs to the map mode (map_mode=True)")
    if map_view_guard is not None and not map_mode:
        raise ValueError("map_view_guard belongs to the map mode (map_mode=True)")
    if map_free_rho is not None and not map_mode:
        raise ValueError("map_free_rho belongs to the map mode (map_mode=True)")
    if map_evict and not map_mode:
        raise ValueError("map_evict belongs to the map mode (map_mode=True)")
    reloc = {k: v for k, v in (("reloc_min_agree", map_reloc_min_agree), ("reloc_rot_deg", map_reloc_rot_deg),
                               ("reloc_trans", map_reloc_trans), ("reloc_align_top", map_reloc_align_top))
             if v is not None}
    if (map_reloc or reloc) and not map_mode:
        raise ValueError("map_reloc belongs to the map mode (map_mode=True)")
    if reloc and not map_reloc:
        raise ValueError(f"{', '.join('map_' + k for k in reloc)}: options of map_reloc=True")
    keyframes = {k: v for k, v in (("keyframe_rot_deg", map_keyframe_rot_deg), ("keyframe_trans", map_keyframe_trans))
                 if v is not None}
    if (map_keyframes or keyframes) and not map_reloc:
        raise ValueError("map_keyframes belongs to the relocalisation (map_reloc=True)")
    if keyframes and not map_keyframes:
        raise ValueError(f"{', '.join('map_' + k for k in keyframes)}: options of map_keyframes=True")
    if (map_refine or map_refine_max_weight is not None) and not map_mode:
        raise ValueError("map_refine belongs to the map mode (map_mode=True)")
    if map_refine_max_weight is not None and not map_refine:
        raise ValueError("map_refine_max_weight: an option of map_refine=True")
    if map_info and not map_mode:
        raise ValueError("map_info belongs to the map mode (map_mode=True)")
    if map_origins and not map_mode:
        raise ValueError("map_origins belongs to the map mode (map_mode=True)")
    if (map_loop or map_loop_min_gap is not None) and not map_mode:
        raise ValueError("map_loop belongs to the map mode (map_mode=True)")
    if map_loop_min_gap is not None and not map_loop:
        raise ValueError("map_loop_min_gap: an option of map_loop=True")
    if (map_photo_scale is not None or map_photo_max_residual is not None) and not map_mode:
        raise ValueError("map_photo_scale belongs to the map mode (map_mode=True)")
    if map_photo_max_residual is not None and map_photo_scale is None:
        raise ValueError("map_photo_max_residual: an option of map_photo_scale")
    if map_photo_scale is not None and not (map_info or map_align or map_loop):
        raise ValueError("map_photo_scale: the photometric term of map_info, map_align or map_loop -- one of them")
    if map_photo_exposure and map_photo_scale is None:
        raise ValueError("map_photo_exposure: an option of map_photo_scale")
    if (map_align_levels is not None or map_align_level_steps is not None) and not map_mode:
        raise ValueError("map_align_levels belongs to the map mode (map_mode=True)")
    if map_align_level_steps is not None and map_align_levels is None:
        raise ValueError("map_align_level_steps: an option of map_align_levels")
    if map_align_levels is not None and not (map_align or map_loop):
        raise ValueError("map_align_levels: the pyramid of the alignments of map_align or map_loop -- one of them")
    pyramid = None
    if map_align_levels is not None:
        pyramid = dict(align_levels=map_align_levels, **({} if map_align_level_steps is None else
                                                         {"align_level_steps": map_align_level_steps}))
    photo_term = None
    if map_photo_scale is not None:
        photo_term = dict(photo_scale=map_photo_scale, **({} if map_photo_max_residual is None else
                                                          {"photo_max_residual": map_photo_max_residual}),
                          **({"photo_exposure": True} if map_photo_exposure else {}))
    loop = None
    if map_loop:
        loop = dict(loop=True, **({} if map_loop_min_gap is None else {"loop_min_gap": map_loop_min_gap}))
    if (map_align or map_align_steps is not None) and not map_mode:
        raise ValueError("map_align belongs to the map mode (map_mode=True)")
    if map_align_steps is not None and not map_align:
        raise ValueError("map_align_steps: an option of map_align=True")
    if map_align_accept and not map_align:
        raise ValueError("map_align_accept: an option of map_align=True")
    align = None
    if map_align:
        align = dict(align=True, **({} if map_align_steps is None else {"align_steps": map_align_steps}),
                     **({"align_accept": True} if map_align_accept else {}))
    refine = None
    if map_refine:
        refine = dict(refine=True, **({} if map_refine_max_weight is None else
                                      {"refine_max_weight": map_refine_max_weight}))
    if sequential:
        return evaluate_sequential(parser, cfg, max_frames, verbose, motion, map_mode, map_capacity, map_view_guard,
                                   map_free_rho, map_free_window, map_evict, map_merge_voxel, map_merge_every,
                                   dict(reloc, reloc=True) if map_reloc else None,
                                   dict(keyframes, keyframes=True) if map_keyframes else None, map_refine=refine,
                                   map_info=bool(map_info), map_align=align, map_origins=bool(map_origins) or bool(map_loop),
                                   map_loop=loop, map_view_occlusion=occlusion or None, map_photo=photo_term,
                                   map_pyramid=pyramid)
    if map_mode:
        raise ValueError("map_mode belongs to the sequential protocol (sequential=True)")
    photo = rgb_lambda != 0.0
    phases = {} if profile else None
    parser.phase_seconds = phases

    def tick():
        if profile:
            torch.cuda.synchronize()
        return time.perf_counter()

    tracker = None
    eTs, eRs, steps = [], [], []
    long_frames = 0  # frames with a tile list long enough to be split over workgroups (a pile of invalid-depth points)
    t0 = time.perf_counter()
    n = len(parser) if max_frames is None else min(len(parser), max_frames)
    for i in range(n):
        d = parser[i]
        H, W = d.src_depth.shape[1:3]
        if tracker is None or tracker.N != d.tar_points.shape[0]:
            # expected depth only: the reference's loop asks for "RGB+ED" (model.py:195-213) and reads renders[..., 3:4]
            # alone (gs_trainer_total.py:104-123) -- the SH colours, their records and three of four composited channels
            # are work whose result nobody looks at.  Same depth, same loss, same pose; 2 % more
            # iterations per second at 102 k Gaussians, 20 % at 816 k.  render_mode="RGB+ED" is the literal call, and
            # what the photometric term needs.
            tracker = GraphTracker(d.tar_points.shape[0], W, H, cfg, device=d.tar_points.device,
                                   render_mode="RGB+ED" if photo else "ED")
        ta = tick()
        scales = init_gs_scales(d.tar_points)
        tb = tick()
        tracker.load_frame(d.tar_points, d.colors, scales, d.src_depth, d.tar_c2w, d.src_c2w, parser.K,
                           pixels=d.pixels if photo else None)
        tc = tick()
        res = tracker.run()
        if profile:
            td = tick()
            for k, v in (("knn_scales", tb - ta), ("load_frame_calibrate", tc - tb), ("optimise", td - tc)):
                phases[k] = phases.get(k, 0.0) + v
        long_frames += int(tracker.rc.long_min > 0)
        # early stop never fired before min_step: fall back to the last iterate's errors, as the reference would log inf
        eTs.append(res.best_eT)
        eRs.append(res.best_eR)
        steps.append(res.steps)
        if verbose:
            print(f"frame {i}: steps {res.steps} loss {res.best_loss:.3e} eT {res.best_eT:.3e} eR {res.best_eR:.3e}")
    dt = time.perf_counter() - t0
    parser.phase_seconds = None
    finite = [(a, b) for a, b in zip(eTs, eRs) if math.isfinite(a) and math.isfinite(b)]
    if not finite:  # e.g. num_iters <= 101: the minimum-loss read-out starts after step 100 and never fired
        return {"ATE": float("nan"), "AAE": float("nan"), "frames": n, "frames_with_result": 0,
                "mean_steps": sum(steps) / max(len(steps), 1), "seconds": dt, "frames_per_s": n / dt if dt > 0 else None,
                "error": "no frame produced a minimum-loss read-out (num_iters must exceed 101)"}
    return {"ATE": rmse([a for a, _ in finite]), "AAE": rmse([b for _, b in finite]), "frames": n,
            "frames_with_result": len(finite), "mean_steps": sum(steps) / max(len(steps), 1),
            "frames_with_long_lists": long_frames, "seconds": dt, "frames_per_s": n / dt if dt > 0 else None,
            **({"phase_seconds": phases} if profile else {})}


def evaluate_sequential(parser: Parser, cfg: TrackerConfig, max_frames: Optional[int] = 1998, verbose: bool = False,
                        motion: str = "constant_velocity", map_mode: bool = False,
                        map_capacity: Optional[int] = None, map_view_guard: Optional[float] = None,
                        map_free_rho: Optional[float] = None, map_free_window: int = 1,
                        map_evict: bool = False, map_merge_voxel: Optional[float] = None,
                        map_merge_every: int = 1, map_reloc: Optional[Dict] = None,
                        map_keyframes: Optional[Dict] = None, map_refine: Optional[Dict] = None,
                        map_info: bool = False, map_align: Optional[Dict] = None, map_origins: bool = False,
                        map_loop: Optional[Dict] = None, map_view_occlusion: Optional[Dict] = None,
                        map_photo: Optional[Dict] = None, map_pyramid: Optional[Dict] = None) -> Dict:
    """Frames 1..n of the room tracked by a Localizer that was given the ground-truth pose of frame 0 and nothing else.
    ATE / AAE: RMSE of the absolute translation / rotation errors of frames 1..n against ground truth, no alignment.
    map_mode: Localizer(mode="map"); the report gains map_gaussians (live points at the end), added_per_frame,
    tracked_per_frame (rows the tracker saw) and map_full (some frame's points were dropped at map_capacity).
    map_view_guard: MapConfig.view_guard_px; the report gains view_violations_per_frame.  map_free_rho /
    map_free_window: MapConfig.free_rho / free_window_px; the report gains removed_per_frame.  map_evict:
    MapConfig.evict; the report gains evicted_per_frame.  map_merge_voxel / map_merge_every: MapConfig.merge_voxel /
    merge_every; the report gains merged_per_frame and merged_at_reset (rows the first frame's own merge removed).
    map_reloc: the MapConfig fields of relocalisation (reloc=True and any of reloc_min_agree, reloc_rot_deg,
    reloc_trans); the report gains relocalised_frames and agree_share_per_frame (agree / (agree + front) of the
    estimate that was kept, None where no row was judged).  map_keyframes: the MapConfig fields of place recognition
    (keyframes=True and any of keyframe_rot_deg, keyframe_trans); the report gains keyframes (those the map holds at the
    end) and recognised_frames (frames that a keyframe's neighbourhood was accepted from).  map_refine: the MapConfig
    fields of refinement (refine=True and, where wanted, refine_max_weight); the report gains refined_per_frame.  map_info: MapConfig.info; every frame prints
    the standard deviations of its pose, the rows used, the smallest eigenvalue of H / used and the verdict, and the report
    gains sigma_t_per_frame (metres), sigma_r_per_frame (degrees), info_used_per_frame, info_min_eig_per_frame and
    weak_frames (None in the lists for a lost frame, which is not asked).  map_align: the MapConfig fields of pose
    alignment (align=True and, where wanted, align_steps); every frame prints what the alignment did, and the report gains
    aligned_per_frame (the aligned start was taken), align_steps_per_frame, align_status_per_frame, aligned_frames, and
    the translation errors motion_eT_per_frame / start_eT_per_frame of the motion model's pose and of the pose the
    tracker started from.  map_origins: MapConfig.origins, every row carries the index of the frame that appended it; the
    report gains origins_non_decreasing (checked after every frame) and rows_per_origin (the live rows at the end that
    came from frame 0, 1, ...).  No correction is applied: that is the caller's decision (``Localizer.close_loop``) --
    unless map_loop: MapConfig fields of the loop closure in ``track()`` (loop=True and, where wanted, loop_min_gap; it
    needs map_origins); every frame that attempts a loop prints what became of it, and the report gains
    loop_status_per_frame, loop_closures (the frames that closed a loop), loop_anchors (the frame each of those edges
    starts at), loop_edge_residuals (of every kept edge after the last solve) and ate_corrected (the RMSE of the final,
    corrected trajectory's translation errors; ATE is that of the estimates as they were made).  map_view_occlusion: the
    MapConfig fields of occlusion culling (view_occlusion_rho and, where wanted, view_occlusion_cell_px /
    view_occlusion_window; it needs map_view_guard); the report gains view_culled_per_frame.  map_photo: the MapConfig
    fields of the photometric term (photo_scale and, where wanted, photo_max_residual; it needs map_info, map_align or
    map_loop); the report gains photo_scale and, with map_info, info_photo_used_per_frame.  map_pyramid: the MapConfig
    fields of the coarse-to-fine alignment (align_levels and, where wanted, align_level_steps; it needs map_align or
    map_loop); the report gains align_levels and, with map_align, align_level_steps_per_frame (the steps every level
    applied, coarse to fine)."""
    n = len(parser) if max_frames is None else min(len(parser), max_frames)
    depth, rgb, pose = parser.frame(0)
    H, W = depth.shape
    extra = {}
    if map_mode:
        extra = dict(mode="map", map_config=MapConfig(capacity=map_capacity, view_guard_px=map_view_guard,
                                                       free_rho=map_free_rho, free_window_px=map_free_window,
                                                       evict=bool(map_evict), merge_voxel=map_merge_voxel,
                                                       merge_every=map_merge_every, **(map_reloc or {}),
                                                       **(map_keyframes or {}), **(map_refine or {}),
                                                       info=bool(map_info), **(map_align or {}),
                                                       origins=bool(map_origins), **(map_loop or {}),
                                                       **(map_view_occlusion or {}), **(map_photo or {}),
                                                       **(map_pyramid or {})))
    loc = Localizer(parser.K, W, H, cfg, normalize=parser.normalize, motion=motion, device=parser.device, **extra)
    t0 = time.perf_counter()
    loc.reset(depth, rgb, pose)
    merged_at_reset = loc.merged_at_reset
    eTs, eRs, steps, lost, path, last_t = [], [], [], 0, 0.0, pose[:3, 3]
    added, tracked, violations, removed, evicted, merged = [], [], [], [], [], []
    culled = []
    relocalised, shares, recognised, refined = 0, [], 0, []
    sigma_t, sigma_r, info_used, info_eig, weak = [], [], [], [], 0
    photo_used = []
    aligned, align_steps, align_status, motion_eT, start_eT = [], [], [], [], []
    level_steps = []
    direct, direct_reason, reloc_aligned = [], [], []
    ordered = True
    exposures = []
    loop_status, closures, anchors, gts = [], [], [], [pose]
    for i in range(1, n + 1):
        depth, rgb, pose = parser.frame(i)
        r = loc.track(depth, rgb, gt_c2w=pose)
        eTs.append(r.eT)
        eRs.append(r.eR)
        steps.append(r.steps)
        lost += int(r.lost)
        added.append(r.added)
        tracked.append(r.tracked)
        violations.append(r.view_violations)
        culled.append(r.view_culled)
        removed.append(r.removed)
        evicted.append(r.evicted)
        merged.append(r.merged)
        refined.append(r.refined)
        if map_reloc:
            relocalised += int(r.relocalised)
            shares.append(r.agree / (r.agree + r.front) if r.agree + r.front > 0 else None)
        if map_keyframes:
            recognised += int(r.recognised >= 0)
        if map_photo and map_photo.get("photo_exposure"):
            exposures.append((r.exposure_gain, r.exposure_offset, r.exposure_status, r.exposure_used))
            print(f"frame {i}: exposure: gain {r.exposure_gain:.5f} offset {r.exposure_offset:.5f} {r.exposure_status} "
                  f"rows used {r.exposure_used}")
        if map_info:
            sigma_t.append(r.sigma_t)
            sigma_r.append(r.sigma_r)
            info_used.append(r.info_used)
            info_eig.append(r.info_min_eig)
            photo_used.append(r.info_photo_used)
            weak += int(bool(r.weak))
            if r.weak is None:
                print(f"frame {i}: pose information: lost, not asked")
            else:
                sig = "none" if r.cov is None else f"sigma_t {r.sigma_t:.3e} m sigma_r {r.sigma_r:.3e} deg"
                print(f"frame {i}: pose information: {sig} rows used {r.info_used} min eig {r.info_min_eig:.3e} "
                      f"weak {r.weak}" + (f" photometric rows {r.info_photo_used}" if map_photo else ""))
        if map_align:
            aligned.append(bool(r.aligned))
            align_steps.append(r.align_steps)
            align_status.append(r.align_status)
            level_steps.append(r.align_level_steps)
            gt_t = pose[:3, 3].to(r.init_c2w.device)
            motion_eT.append(float(torch.norm(r.align_from[:3, 3] - gt_t)))
            start_eT.append(float(torch.norm(r.init_c2w[:3, 3] - gt_t)))
            print(f"frame {i}: pose alignment: {r.align_status} after {r.align_steps} steps"
                  + (f" (per level {r.align_level_steps})" if r.align_level_steps is not None else "") + f", moved {r.align_moved_t:.3e} m "
                  f"{r.align_moved_r_deg:.3e} deg, taken {r.aligned}: start eT {motion_eT[-1]:.3e} -> {start_eT[-1]:.3e}"
                  + ("" if r.direct is None else f", direct {r.direct}" + (f" ({r.direct_reason})" if r.direct_reason else "")))
            direct.append(r.direct)
            direct_reason.append(r.direct_reason)
        if map_reloc and map_reloc.get("reloc_align_top"):
            reloc_aligned.append(r.reloc_aligned)
        if map_loop:
            gts.append(pose)
            loop_status.append(r.loop_status)
            if r.loop:
                closures.append(i)
                anchors.append(r.loop_anchor)
            if r.loop_status not in (None, "waiting"):
                moved = "" if r.loop_moved_t is None else f", moved {r.loop_moved_t:.3e} m {r.loop_moved_r_deg:.3e} deg"
                print(f"frame {i}: loop: {r.loop_status}, {r.loop_old_tested} old rows tested{moved}"
                      + (f", anchor {r.loop_anchor}, {r.loop_correction.moved} rows moved" if r.loop else ""))
        if map_origins:
            o = loc.map.origins[: loc.map.n_live]
            ordered = ordered and bool((o[1:] >= o[:-1]).all())
        path += float(torch.norm(pose[:3, 3] - last_t))
        last_t = pose[:3, 3]
        if verbose:
            loss = "none" if r.best_loss is None else f"{r.best_loss:.3e}"  # a direct frame has no loss
            print(f"frame {i}: steps {r.steps} best step {r.best_step} loss {loss} eT {r.eT:.3e} eR {r.eR:.3e}")
    dt = time.perf_counter() - t0
    return {"mode": "sequential", "motion": motion, "ATE": rmse(eTs), "AAE": rmse(eRs),
            "final_eT": eTs[-1] if eTs else float("nan"), "final_eR": eRs[-1] if eRs else float("nan"),
            "path_length": path, "frames": n, "lost_frames": lost, "mean_steps": sum(steps) / max(len(steps), 1),
            "seconds": dt, "frames_per_s": n / dt if dt > 0 else None,
            **({"map_gaussians": loc.map.n_live, "added_per_frame": added, "tracked_per_frame": tracked,
                "map_full": loc.map.full} if map_mode else {}),
            **({"view_guard_px": map_view_guard, "view_violations_per_frame": violations}
               if map_view_guard is not None else {}),
            **({**map_view_occlusion, "view_culled_per_frame": culled} if map_view_occlusion else {}),
            **({"free_rho": map_free_rho, "free_window_px": map_free_window, "removed_per_frame": removed}
               if map_free_rho is not None else {}),
            **({"evict": True, "evicted_per_frame": evicted} if map_evict else {}),
            **({"merge_voxel": map_merge_voxel, "merge_every": map_merge_every, "merged_per_frame": merged,
                "merged_at_reset": merged_at_reset} if map_merge_voxel is not None else {}),
            **({"reloc": True, "relocalised_frames": relocalised, "agree_share_per_frame": shares} if map_reloc else {}),
            **({"keyframes": loc.map.n_keyframes, "recognised_frames": recognised} if map_keyframes else {}),
            **({"refine": True, "refined_per_frame": refined} if map_refine else {}),
            **({"info": True, "sigma_t_per_frame": sigma_t, "sigma_r_per_frame": sigma_r,
                "info_used_per_frame": info_used, "info_min_eig_per_frame": info_eig, "weak_frames": weak}
               if map_info else {}),
            **({**map_photo, **({"info_photo_used_per_frame": photo_used} if map_info else {}),
                **({"exposure_per_frame": exposures} if map_photo.get("photo_exposure") else {})} if map_photo else {}),
            **({**map_pyramid, **({"align_level_steps_per_frame": level_steps} if map_align else {})}
               if map_pyramid else {}),
            **({"align": True, "aligned_per_frame": aligned, "align_steps_per_frame": align_steps,
                "align_status_per_frame": align_status, "aligned_frames": sum(aligned),
                "motion_eT_per_frame": motion_eT, "start_eT_per_frame": start_eT} if map_align else {}),
            **({"align_accept": True, "direct_per_frame": direct, "direct_reason_per_frame": direct_reason,
                "direct_frames": sum(bool(d) for d in direct)} if map_align and map_align.get("align_accept") else {}),
            **({"reloc_align_top": map_reloc["reloc_align_top"], "reloc_aligned_per_frame": reloc_aligned}
               if map_reloc and map_reloc.get("reloc_align_top") else {}),
            **({"origins": True, "origins_non_decreasing": ordered,
                "rows_per_origin": torch.bincount(loc.map.origins[: loc.map.n_live].long().cpu(),
                                                  minlength=n + 1).tolist()} if map_origins else {}),
            **({"loop": True, "loop_status_per_frame": loop_status, "loop_closures": closures, "loop_anchors": anchors,
                "loop_edge_residuals": ([] if loc.last_pose_graph is None
                                        else [float(v) for v in loc.last_pose_graph.loop_residuals]),
                "ate_corrected": float(torch.sqrt(torch.mean(torch.stack(
                    [torch.sum((a[:3, 3].cpu() - b[:3, 3].cpu()) ** 2) for a, b in zip(loc.trajectory[1:], gts[1:])]))))
                } if map_loop else {})}


def main(argv=None):
    ap = argparse.ArgumentParser(description="GsplatLoc evaluation on the MI355X rasterizer")
    ap.add_argument("--dataset", choices=["Replica", "TUM"], default="Replica")
    ap.add_argument("--rooms", nargs="+", default=["room0"])
    ap.add_argument("--root", required=True, help="dataset root (contains <room>/ for Replica, rgbd_dataset_* for TUM)")
    ap.add_argument("--num-iters", type=int, default=2000)
    ap.add_argument("--max-frames", type=int, default=1998)
    ap.add_argument("--no-normalize", action="store_true")
    ap.add_argument("--out", default="res.json")
    ap.add_argument("--verbose", action="store_true")
    ap.add_argument("--rgb-lambda", type=float, default=0.0,
                    help="weight of the photometric term (RGB L1 + SSIM against the frame's image); 0 = off")
    ap.add_argument("--ssim-lambda", type=float, default=0.5, help="share of 1 - SSIM inside the photometric term")
    ap.add_argument("--sequential", action="store_true",
                    help="track each room from the ground-truth pose of frame 0 only and report the trajectory's drift")
    ap.add_argument("--motion", choices=["hold", "constant_velocity"], default="constant_velocity",
                    help="--sequential: where a frame's optimisation starts (the previous estimate, or the "
                         "constant-velocity prediction of the last two)")
    ap.add_argument("--map", action="store_true",
                    help="--sequential: track every frame against a Gaussian map grown on the device (frame to map) "
                         "instead of the previous frame alone")
    ap.add_argument("--map-capacity", type=int, default=None, help="--map: rows of the map (default 4 * W * H)")
    ap.add_argument("--map-view-guard", type=float, default=None, metavar="PX",
                    help="--map: track every frame against the map's points in view from its start pose, the image "
                         "widened by PX pixels on every side (default: against all of them)")
    ap.add_argument("--map-view-occlusion", type=float, default=None, metavar="RHO",
                    help="--map-view-guard: leave out the points in view that nearer points of the map hide, those more "
                         "than this fraction behind the nearest depth of every z-buffer cell around their own "
                         "(default: the frustum is the only test)")
    ap.add_argument("--map-view-occlusion-cell", type=int, default=None, metavar="PX",
                    help="--map-view-occlusion: the side of a z-buffer cell, 1, 2, 4, 8 or 16 pixels (default 4)")
    ap.add_argument("--map-view-occlusion-window", type=int, default=None, metavar="N",
                    help="--map-view-occlusion: the cells around a point's cell that must all hold a nearer depth, "
                         "0 .. 3 (default 1)")
    ap.add_argument("--map-free-rho", type=float, default=None, metavar="RHO",
                    help="--map: after every frame's insertion remove the map's points that the frame sees through, "
                         "those more than this fraction in front of everything it observes around their pixel "
                         "(default: the map only grows)")
    ap.add_argument("--map-free-window", type=int, default=1, metavar="PX",
                    help="--map-free-rho: the pixels around a point's pixel that must all lie behind it (0 .. 3)")
    ap.add_argument("--map-evict", action="store_true",
                    help="--map: a bounded map -- a frame whose new points do not fit in --map-capacity first evicts "
                         "the least recently observed points (default: they are dropped and the map is full)")
    ap.add_argument("--map-merge-voxel", type=float, default=None, metavar="M",
                    help="--map: a map with a resolution -- the points that share a cube of side M metres are fused into "
                         "one after a frame's insertion (default: every inserted point stays one point)")
    ap.add_argument("--map-merge-every", type=int, default=1, metavar="K",
                    help="--map-merge-voxel: fuse after every K-th frame")
    ap.add_argument("--map-reloc", action="store_true",
                    help="--map: relocalisation -- an estimate the map does not confirm is tracked once more, from the "
                         "best-scoring pose of a grid around the frame's start poses; rejected again, the frame is lost "
                         "and leaves the map alone (default: every estimate with a recorded minimum is inserted)")
    ap.add_argument("--map-reloc-min-agree", type=float, default=None, metavar="S",
                    help="--map-reloc: least share of the judged map points that must lie on the observed surface")
    ap.add_argument("--map-reloc-rot-deg", type=float, default=None, metavar="D",
                    help="--map-reloc: rotation step of the candidate grid, degrees")
    ap.add_argument("--map-reloc-trans", type=float, default=None, metavar="M",
                    help="--map-reloc: translation step of the candidate grid, metres")
    ap.add_argument("--map-keyframes", action="store_true",
                    help="--map-reloc: place recognition -- a frame that stays lost is compared with the keyframes of "
                         "the map, and tracked once more from the best-scoring pose around the most similar ones")
    ap.add_argument("--map-keyframe-rot-deg", type=float, default=None, metavar="D",
                    help="--map-keyframes: a frame further than D degrees from every keyframe becomes one")
    ap.add_argument("--map-keyframe-trans", type=float, default=None, metavar="M",
                    help="--map-keyframes: a frame further than M metres from every keyframe becomes one")
    ap.add_argument("--map-refine", action="store_true",
                    help="--map: refinement -- the map's points that a frame observes again move along their ray to the "
                         "running mean of the depths observed there (default: a point keeps its first depth)")
    ap.add_argument("--map-refine-max-weight", type=int, default=None, metavar="N",
                    help="--map-refine: the number of depths from which on the mean is an exponential one (default 64)")
    ap.add_argument("--map-origins", action="store_true",
                    help="--map: every point of the map carries the index of the frame that appended it, so that the map "
                         "can follow a corrected trajectory; the report says that the origins stayed non-decreasing in map "
                         "order and how many live points came from each frame (no correction is applied)")
    ap.add_argument("--map-loop", action="store_true",
                    help="--map: loops are closed while tracking -- a frame that sees the points of much older frames again "
                         "is aligned against those alone, and a pose graph over the tracked odometry and every such "
                         "constraint corrects the trajectory and the map (implies --map-origins); the report lists the "
                         "closures and their anchors")
    ap.add_argument("--map-loop-min-gap", type=int, default=None, metavar="G",
                    help="--map-loop: only frames at least G behind the current one count as old (default 30)")
    ap.add_argument("--map-info", action="store_true",
                    help="--map: pose information -- every frame that is not lost prints the standard deviations of its "
                         "pose (metres, degrees) from the map's points against its depth image, the points used, the "
                         "smallest eigenvalue of the information matrix per point and whether the frame is weak; "
                         "nothing is gated on them")
    ap.add_argument("--map-align", action="store_true",
                    help="--map: pose alignment -- every frame's start pose is aligned to the map by Gauss-Newton steps "
                         "on the device before the tracker runs, and taken when the map scores it no worse")
    ap.add_argument("--map-align-steps", type=int, default=None, metavar="K",
                    help="--map-align: iterations per frame, 1 .. 32 (default 8)")
    ap.add_argument("--map-align-accept", action="store_true",
                    help="--map-align: a converged alignment that the map scores no worse than the start and that the "
                         "map's points pin down in every direction is the frame's pose -- the tracker does not run; the "
                         "report counts these direct frames")
    ap.add_argument("--map-reloc-align-top", type=int, default=None, metavar="K",
                    help="--map-reloc: the K best candidates of a relocalisation grid (1 .. 16) are aligned to the map "
                         "in one call before the winner is chosen (default 0: none)")
    ap.add_argument("--map-photo-scale", type=float, default=None, metavar="S",
                    help="--map-info / --map-align / --map-loop: a photometric term in their normal equations -- every "
                         "point that gives a depth equation also gives one from its colour against the frame's image, S "
                         "metres per unit of intensity (0 .. 16; 0.2 is the documented value to start from)")
    ap.add_argument("--map-photo-max-residual", type=float, default=None, metavar="R",
                    help="--map-photo-scale: a point whose intensity misses the image's by more than R gives no "
                         "photometric equation (0 .. 1, default 0.1)")
    ap.add_argument("--map-photo-exposure", action="store_true",
                    help="--map-photo-scale: exposure compensation -- every frame's gain and offset are estimated against "
                         "the map and its image is corrected before the photometric term, the refinement and the "
                         "insertion read it (default: every frame is taken to have the first frame's exposure)")
    ap.add_argument("--map-align-levels", type=int, default=None, metavar="L",
                    help="--map-align / --map-loop: coarse-to-fine alignment -- every frame builds an image pyramid of L "
                         "levels (1 .. 4) once, and its alignments start at the coarsest level: every level doubles the "
                         "distance from which the photometric term converges (default 0: the frame alone)")
    ap.add_argument("--map-align-level-steps", type=int, default=None, metavar="K",
                    help="--map-align-levels: iterations at every coarse level, 1 .. 32 (default: those of the frame)")
    a = ap.parse_args(argv)
    if a.map_merge_voxel is not None and not a.map:
        ap.error("--map-merge-voxel needs --map")
    if a.map_merge_every != 1 and a.map_merge_voxel is None:
        ap.error("--map-merge-every needs --map-merge-voxel")
    if a.map and not a.sequential:
        ap.error("--map needs --sequential")
    if a.map_view_guard is not None and not a.map:
        ap.error("--map-view-guard needs --map")
    if a.map_view_occlusion is not None and a.map_view_guard is None:
        ap.error("--map-view-occlusion needs --map-view-guard")
    for flag, value in (("--map-view-occlusion-cell", a.map_view_occlusion_cell),
                        ("--map-view-occlusion-window", a.map_view_occlusion_window)):
        if value is not None and a.map_view_occlusion is None:
            ap.error(f"{flag} needs --map-view-occlusion")
    if a.map_free_rho is not None and not a.map:
        ap.error("--map-free-rho needs --map")
    if a.map_evict and not a.map:
        ap.error("--map-evict needs --map")
    if a.map_free_window != 1 and not a.map:
        ap.error("--map-free-window needs --map")
    if a.map_reloc and not a.map:
        ap.error("--map-reloc needs --map")
    for flag, value in (("--map-reloc-min-agree", a.map_reloc_min_agree), ("--map-reloc-rot-deg", a.map_reloc_rot_deg),
                        ("--map-reloc-trans", a.map_reloc_trans)):
        if value is not None and not a.map:
            ap.error(f"{flag} needs --map")
        if value is not None and not a.map_reloc:
            ap.error(f"{flag} needs --map-reloc")
    if a.map_keyframes and not a.map_reloc:
        ap.error("--map-keyframes needs --map-reloc")
    for flag, value in (("--map-keyframe-rot-deg", a.map_keyframe_rot_deg), ("--map-keyframe-trans", a.map_keyframe_trans)):
        if value is not None and not a.map_keyframes:
            ap.error(f"{flag} needs --map-keyframes")
    if a.map_refine and not a.map:
        ap.error("--map-refine needs --map")
    if a.map_refine_max_weight is not None and not a.map_refine:
        ap.error("--map-refine-max-weight needs --map-refine")
    if a.map_info and not a.map:
        ap.error("--map-info needs --map")
    if a.map_origins and not a.map:
        ap.error("--map-origins needs --map")
    if a.map_loop and not a.map:
        ap.error("--map-loop needs --map")
    if a.map_loop_min_gap is not None and not a.map_loop:
        ap.error("--map-loop-min-gap needs --map-loop")
    if a.map_align and not a.map:
        ap.error("--map-align needs --map")
    if a.map_align_steps is not None and not a.map_align:
        ap.error("--map-align-steps needs --map-align")
    if a.map_align_accept and not a.map_align:
        ap.error("--map-align-accept needs --map-align")
    if a.map_reloc_align_top is not None and not a.map_reloc:
        ap.error("--map-reloc-align-top needs --map-reloc")
    if a.map_photo_scale is not None and not (a.map_info or a.map_align or a.map_loop):
        ap.error("--map-photo-scale needs --map-info, --map-align or --map-loop")
    if a.map_photo_max_residual is not None and a.map_photo_scale is None:
        ap.error("--map-photo-max-residual needs --map-photo-scale")
    if a.map_photo_exposure and a.map_photo_scale is None:
        ap.error("--map-photo-exposure needs --map-photo-scale")
    if a.map_align_levels is not None and not (a.map_align or a.map_loop):
        ap.error("--map-align-levels needs --map-align or --map-loop")
    if a.map_align_level_steps is not None and a.map_align_levels is None:
        ap.error("--map-align-level-steps needs --map-align-levels")
    out = {}
    for room in a.rooms:
        parser = Parser(a.dataset, room, normalize=not a.no_normalize, input_folder=a.root)
        r = evaluate_room(parser, a.num_iters, a.max_frames, a.verbose, rgb_lambda=a.rgb_lambda,
                          ssim_lambda=a.ssim_lambda, sequential=a.sequential, motion=a.motion, map_mode=a.map,
                          map_capacity=a.map_capacity, map_view_guard=a.map_view_guard,
                          map_free_rho=a.map_free_rho, map_free_window=a.map_free_window, map_evict=a.map_evict,
                          map_merge_voxel=a.map_merge_voxel, map_merge_every=a.map_merge_every, map_reloc=a.map_reloc,
                          map_reloc_min_agree=a.map_reloc_min_agree, map_reloc_rot_deg=a.map_reloc_rot_deg,
                          map_reloc_trans=a.map_reloc_trans, map_keyframes=a.map_keyframes,
                          map_keyframe_rot_deg=a.map_keyframe_rot_deg, map_keyframe_trans=a.map_keyframe_trans,
                          map_refine=a.map_refine, map_refine_max_weight=a.map_refine_max_weight,
                          map_info=a.map_info, map_align=a.map_align, map_align_steps=a.map_align_steps,
                          map_align_accept=a.map_align_accept, map_reloc_align_top=a.map_reloc_align_top,
                          map_origins=a.map_origins or a.map_loop, map_loop=a.map_loop,
                          map_loop_min_gap=a.map_loop_min_gap, map_view_occlusion=a.map_view_occlusion,
                          map_view_occlusion_cell=a.map_view_occlusion_cell,
                          map_view_occlusion_window=a.map_view_occlusion_window,
                          map_photo_scale=a.map_photo_scale, map_photo_max_residual=a.map_photo_max_residual,
                          map_photo_exposure=a.map_photo_exposure,
                          map_align_levels=a.map_align_levels, map_align_level_steps=a.map_align_level_steps)
        out[room] = {"gsplatloc_amd": r}
        print(room, json.dumps(r))
    with open(a.out, "w") as f:
        json.dump(out, f, indent=2)


if __name__ == "__main__":
    main()
