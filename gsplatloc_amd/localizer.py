"""Sequential localisation: a depth (or RGB-D) sequence tracked from its FIRST pose only.

The evaluation protocol of ``gsplatloc_amd.eval`` places pair (i, i+1) with the ground-truth pose of frame i and starts
there.  ``Localizer`` hands its own estimates on instead:

  1. the Gaussians come from the PREVIOUS frame's depth and colours, placed with the previous frame's ESTIMATED pose;
  2. the target depth is the new frame's;
  3. the optimisation starts from the previous estimate ("hold", and always for the second frame) or from the
     constant-velocity prediction of the last two estimates (``predict_pose`` -- the hand-over the reference declares as
     ``update_pose(None)`` / ``predict_next_pose``, /root/reference/src/my_gsplat/model.py, and never calls);
  4. both are moved into the pair's PCA frame (``AlignData.norm_T``) when ``normalize`` is on;
  5. ``GraphTracker.load_frame`` / ``run``;
  6. the frame's estimate is the MINIMUM-LOSS pose the device kept (``TrackResult.best_c2w``), moved back to the world.

The pair is built by ``data.dataset.build_pair``, the function ``Parser`` uses.  One ``GraphTracker`` is kept while the
number of Gaussians and the image size stay the same.  The host synchronises once per frame anyway (the tracker's poll
and its calibration pass), so the hand-over is host code.

``mode="map"`` replaces step 1: the Gaussians are the live points of a persistent ``GaussianMap`` (mapping.py), already in
the world, which every tracked frame extends by the pixels the map does not explain.  Steps 2 - 6 are unchanged.
With ``MapConfig.view_guard_px`` they are the live points in view from the start pose of step 3, the image widened by
that guard band; after the frame the band is checked against the estimate (``GaussianMap.view_violations``), and where
it did not hold the render the new pixels are judged against is made from a selection at the estimate.
With ``MapConfig.view_occlusion_rho`` the points in view that nearer points of the map hide are left out as well, and the
check at the estimate counts the points visible from there.
With ``MapConfig.free_rho`` the map also shrinks: after the insertion of a frame that is not lost, the live rows that
frame sees through -- in front of everything it observes around their pixel -- are removed
(``GaussianMap.remove_seen_through``).  The hole a removed ghost leaves is filled by the NEXT frame's insertion.
With ``MapConfig.evict`` the map lives in its capacity: before the insertion of a frame that is not lost the rows it
observes are stamped with its index (``GaussianMap.observe``, at the estimate), and an insertion that is short of room
first evicts the least recently observed rows (``GaussianMap.evict``).
With ``MapConfig.merge_voxel`` the map has a resolution: after the first frame's insertion and after the insertion (and
the free-space removal) of every ``merge_every``-th tracked frame that is not lost, the live rows that share a voxel are
fused into one (``GaussianMap.merge``).
With ``MapConfig.reloc`` an estimate has to be confirmed by the map before any of that: the live rows the new frame
tests, confirms and sees through from the estimate are counted (``GaussianMap.score_poses``), and an estimate with too
few rows tested, or too small a share of confirmed rows among those confirmed or seen through, is rejected.  The frame
is then tracked once more, from the best-scoring pose of a small grid of turns and shifts around its start poses
(``reloc_candidates``); an estimate rejected again makes the frame a lost one, which leaves the map alone.  This is no
place recognition -- nothing beyond that grid is tried -- and it repairs nothing a wrongly accepted frame has inserted.
With ``MapConfig.keyframes`` place recognition follows: the map keeps the pose and a small descriptor of the depth image
of the frames that built it (``GaussianMap.add_keyframe``), and a frame that the grid leaves lost is compared with all
of them (``GaussianMap.match_place``).  The poses of the most similar keyframes, each turned by the image shift under
which it matched (``place_base``), are the bases of one more grid, which is scored and tracked from as before.
With ``MapConfig.refine`` the map improves where it is seen again: after the insertion render of a frame that is not
lost and before anything is stamped or inserted, the live rows the frame observes where it expects them move along
their ray to the running mean of the depths observed there (``GaussianMap.refine``, at the estimate).
With ``MapConfig.info`` a frame that is not lost also says how well it constrains its pose: after the relocalisation flow
and before anything touches the map, the normal equations of the final estimate are summed over the map's rows against
the frame's depth image (``GaussianMap.pose_information``), and the frame reports the covariance of its pose and whether
it is weak.  Nothing is gated on it.
With ``MapConfig.align`` step 3 looks at the frame: the motion model's start pose is aligned to the map by a few
Gauss-Newton steps on those normal equations, iterated on the device (``GaussianMap.align_pose``), and the aligned pose
is what the frame starts from when the map scores it no worse than the motion model's (``GaussianMap.score_poses``).
With ``MapConfig.align_accept`` that alignment may be the whole frame: it goes through ``GaussianMap.align_poses``, which
leaves the normal equations at the aligned pose, and an alignment that converged, that the map scores no worse than the
start and that enough rows pin down in every direction is the frame's estimate -- the tracker does not run
(``LocalizeResult.direct``).  With ``MapConfig.reloc_align_top`` the best candidates of a relocalisation grid are aligned
the same way, in one call, before the winner is chosen.
With ``MapConfig.origins`` the map can follow a corrected trajectory: every row carries the index its frame's pose has
in ``trajectory``, and ``correct_trajectory`` (any new poses) or ``close_loop`` (one constraint on one frame, spread over
the frames of the loop) moves the rows, the keyframe poses and the poses themselves (``GaussianMap.correct``).  Neither
is called by ``track``: when a loop is closed is the caller's decision -- unless
``MapConfig.loop`` is on: then ``track`` looks for a loop itself.  Every ``loop_every``-th frame that is not lost, before
anything touches the map, is held against the rows of the frames at least ``loop_min_gap`` behind it
(``GaussianMap.covisibility``, ``loop_constraint``); an alignment against those rows alone that converged, agrees with
them and moved the estimate becomes a loop edge (``add_loop``) of a pose graph over the tracked odometry and every edge
so far (``optimise_pose_graph``), and the trajectory and the map follow its solution.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Callable, List, Optional

import numpy as np
import torch
from torch import Tensor

from .data.dataset import build_pair
from .data.normalize import denormalize_camera, transform_cameras
from .mapping import INFO_MIN_EIG, SCORE_MAX_POSES, GaussianMap, MapConfig, optimise_pose_graph, spread_correction
from .my_gsplat.geometry import construct_full_pose, depth_to_points, init_gs_scales, render_depth_alpha
from .my_gsplat.trainer import TrackerConfig, TrackResult, calculate_rotation_error, calculate_translation_error
from .my_gsplat.transform import normalize_quaternion, quat_to_rotation_matrix, rotation_matrix_to_quaternion

MOTIONS = ("constant_velocity", "hold")
MODES = ("frame", "map")


@torch.no_grad()
def predict_pose(prev_c2w: Tensor, cur_c2w: Tensor) -> Tensor:
    """Constant velocity in parameter space, on two world poses: q = normalise(q_cur + (q_cur - q_prev)) on wxyz
    quaternions, t = t_cur + (t_cur - t_prev).  q and -q are the same rotation and two independent conversions may land
    on opposite hemispheres, so q_prev is negated when its dot product with q_cur is negative (differencing them as they
    come would extrapolate to a rotation about 180 degrees away)."""
    q_prev = rotation_matrix_to_quaternion(prev_c2w[:3, :3].contiguous())
    q_cur = rotation_matrix_to_quaternion(cur_c2w[:3, :3].contiguous())
    if float((q_prev * q_cur).sum()) < 0.0:
        q_prev = -q_prev
    q = normalize_quaternion(q_cur + (q_cur - q_prev))
    t = cur_c2w[:3, 3] + (cur_c2w[:3, 3] - prev_c2w[:3, 3])
    return construct_full_pose(quat_to_rotation_matrix(q), t)


@dataclass
class LocalizeResult:
    c2w: Tensor  # [4,4] the frame's estimate in the world: the minimum-loss pose (the last iterate when lost)
    init_c2w: Tensor  # [4,4] the pose the optimisation started from, in the world
    steps: int
    best_step: int
    best_loss: Optional[float]  # None on a direct frame (align_accept)
    lost: bool  # no minimum was ever recorded (best_step == -1)
    eT: Optional[float] = None  # metres / degrees against gt_c2w, when one was given
    eR: Optional[float] = None
    map_size: Optional[int] = None  # mode="map": live map points after this frame, and how many it added
    added: Optional[int] = None
    tracked: Optional[int] = None  # mode="map": rows the tracker saw (all live rows, or those in the guarded view)
    view_violations: Optional[int] = None  # view_guard_px: rows in reach of the view from c2w that were not tracked
    view_culled: Optional[int] = None  # view_occlusion_rho: rows of the tracked band left out as hidden by nearer rows
    removed: Optional[int] = None  # free_rho: live rows this frame saw through, removed after its insertion
    evicted: Optional[int] = None  # evict: least recently observed rows that made room for this frame's insertion
    merged: Optional[int] = None  # merge_voxel: rows removed by fusing the rows that share a voxel, after the insertion
    # reloc: ``lost`` is "the map does not confirm the estimate" (not accepted, also after a second tracking);
    # relocalised: the estimate is that of a second (keyframes: or third) tracking, started from the best-scoring
    # candidate pose; tested / agree / front: the map's verdict on c2w (GaussianMap.score_poses)
    relocalised: Optional[bool] = None
    tested: Optional[int] = None
    agree: Optional[int] = None
    front: Optional[int] = None
    # keyframes: the slot this frame was kept in as a keyframe after its insertion (None: it was not, or the option is
    # off); recognised: the slot of the keyframe whose turned pose was the base of the candidate that a third tracking
    # was accepted from, -1 on a frame that did not need place recognition or that it did not save (None: option off)
    keyframe: Optional[int] = None
    recognised: Optional[int] = None
    refined: Optional[int] = None  # refine: live rows this frame observed again and moved, before its insertion
    # info (None on a lost frame, which is not asked): cov [6,6] float64 numpy, the covariance sigma^2 H^-1 of the left
    # perturbation (omega [rad], upsilon [m]) of the world-to-camera pose in the camera's frame -- None when weak;
    # sigma_t [m] / sigma_r [deg]: the square roots of the traces of its translation / rotation blocks (None when
    # weak); info_used: the rows the sums were taken over; info_min_eig: the smallest eigenvalue of H / used; weak: fewer
    # than 7 rows used, or that eigenvalue below MapConfig.info_min_eig
    cov: Optional[object] = None
    sigma_t: Optional[float] = None
    sigma_r: Optional[float] = None
    info_used: Optional[int] = None
    info_min_eig: Optional[float] = None
    weak: Optional[bool] = None
    # info with MapConfig.photo_scale: the rows among info_used that also gave a photometric equation (cov, sigma_t,
    # sigma_r, info_min_eig and weak are then those of geometry plus colour)
    info_photo_used: Optional[int] = None
    # MapConfig.photo_exposure: the exposure correction that the frame's image entered the map with -- gain * rgb + 255 *
    # offset, estimated against the map at the frame's final estimate (a lost frame: at its start pose, and nothing
    # entered the map); exposure_status: ``Exposure.status`` -- anything but "OK" is no estimate, and the frame went in
    # as it was: gain 1, offset 0; exposure_used: the rows of the last pass
    exposure_gain: Optional[float] = None
    exposure_offset: Optional[float] = None
    exposure_status: Optional[str] = None
    exposure_used: Optional[int] = None
    # align: aligned -- the start pose the map's Gauss-Newton steps gave was taken (init_c2w is then that pose; False:
    # the alignment refused, or the map scored its pose worse than the motion model's, and the frame ran from that);
    # align_status / align_steps: ``PoseAlignment.status`` / ``steps``; align_from: the motion model's pose [4,4];
    # align_moved_t [m] / align_moved_r_deg: from there to the alignment's pose (0 when it did not move); align_scores:
    # ((tested, agree, front) of the motion model's pose, of the alignment's) that decided, None when it refused
    aligned: Optional[bool] = None
    align_status: Optional[str] = None
    align_steps: Optional[int] = None
    align_from: Optional[Tensor] = None
    align_moved_t: Optional[float] = None
    align_moved_r_deg: Optional[float] = None
    align_scores: Optional[tuple] = None
    # MapConfig.align_levels (None with the option at 0): the steps every level of the start pose's alignment applied,
    # from the coarsest level to the frame itself (``PoseAlignment.level_steps``; align_steps is the last of them)
    align_level_steps: Optional[list] = None
    # align_accept (both None with the option off): direct -- the aligned pose is the frame's estimate and the tracker
    # did not run (steps 0, best_step -1, best_loss None; lost is the map's verdict alone); direct_reason: None on a
    # direct frame, otherwise the first rule that failed -- "status" (the alignment is not CONVERGED), "open" (it
    # converged on its last iteration: no sums at the final pose), "share" (the map scores the start better), "used"
    # (fewer than align_accept_min_used rows in the final sums), "weak" (their smallest eigenvalue is below
    # align_accept_min_eig) -- or "rejected": reloc did not confirm the aligned pose, and the frame was tracked from
    # the motion model's start
    direct: Optional[bool] = None
    direct_reason: Optional[str] = None
    # reloc_align_top (None with the option at 0, or on a frame that needed no retry): the candidates of the last retry
    # whose alignment took their place
    reloc_aligned: Optional[int] = None
    # loop (None with the option off): loop -- this frame closed a loop; loop_status: what the policy ended with, one of
    # ``LOOP_STATUS`` (None on a lost frame, which is not asked); loop_old_tested: the rows of the frames at least
    # loop_min_gap behind that the frame tests from its estimate; loop_anchor: the frame the loop edge starts at;
    # loop_moved_t [m] / loop_moved_r_deg: from the estimate to the pose aligned against the old rows;
    # loop_correction: the ``TrajectoryCorrection`` of the closure.  On a frame that closed a loop c2w is the corrected
    # pose of the frame
    loop: Optional[bool] = None
    loop_status: Optional[str] = None
    loop_old_tested: Optional[int] = None
    loop_anchor: Optional[int] = None
    loop_moved_t: Optional[float] = None
    loop_moved_r_deg: Optional[float] = None
    loop_correction: Optional["TrajectoryCorrection"] = None


@dataclass
class TrajectoryCorrection:
    """What ``Localizer.correct_trajectory`` / ``close_loop`` did.  moved: the map's rows that were moved; outside: the
    rows whose origin lies outside the trajectory (0 for a map this localizer built); frames: the poses whose
    correction D_k = new_k old_k^-1 is not the identity; max_trans [m] / max_rot_deg: the largest translation and the
    largest rotation angle over the D_k."""
    moved: int
    outside: int
    frames: int
    max_trans: float
    max_rot_deg: float


LOOP_STATUS = ("waiting", "few_rows", "not_converged", "rejected", "small", "closed")


def _step(axis: int, rot_deg: float = 0.0, trans: float = 0.0) -> Tensor:
    """float64 [4,4]: a turn by rot_deg degrees about, or a shift by trans along, coordinate axis 0 / 1 / 2."""
    M = torch.eye(4, dtype=torch.float64)
    if rot_deg != 0.0:
        a, b = (axis + 1) % 3, (axis + 2) % 3
        c, s = math.cos(math.radians(rot_deg)), math.sin(math.radians(rot_deg))
        M[a, a], M[a, b], M[b, a], M[b, b] = c, -s, s, c
    M[axis, 3] = trans
    return M


def reloc_candidates(bases, rot_deg: float, trans: float, levels: int) -> Tensor:
    """The candidate start poses of a relocalisation, [k,4,4] float32 on the device of the first base: for every base
    c2w [4,4], in the order given, the base itself; then for level l = 1 .. levels and axis x, y, z the turns
    c2w @ R(axis, +l rot_deg), c2w @ R(axis, -l rot_deg); then for l = 1 .. levels and axis x, y, z the shifts
    c2w @ T(axis, +l trans), c2w @ T(axis, -l trans) -- the camera's own axes, 1 + 12 levels poses per base.  Composed
    in float64 and rounded to float32 once (a base comes back bit for bit).  More poses than one call of
    ``GaussianMap.score_poses`` takes (64) are refused."""
    bases = [torch.as_tensor(b) for b in bases]
    levels = int(levels)
    if not bases or levels < 1:
        raise ValueError("reloc_candidates: at least one base pose and one level")
    if len(bases) * (1 + 12 * levels) > SCORE_MAX_POSES:
        raise ValueError(f"reloc_candidates: {len(bases)} bases x {1 + 12 * levels} poses are more than the "
                         f"{SCORE_MAX_POSES} one scoring call takes")
    out = []
    for b in bases:
        if b.shape != (4, 4):
            raise ValueError(f"a base pose is {tuple(b.shape)}, not (4, 4)")
        c2w = b.detach().cpu().double()
        out.append(c2w)
        for kind in ("rot_deg", "trans"):
            size = float(rot_deg) if kind == "rot_deg" else float(trans)
            for level in range(1, levels + 1):
                for axis in range(3):
                    for sign in (1.0, -1.0):
                        out.append(c2w @ _step(axis, **{kind: sign * level * size}))
    return torch.stack(out).to(dtype=torch.float32, device=bases[0].device)


def place_base(c2w_kf, sx: int, sy: int, width: int, height: int, fx: float, fy: float) -> Tensor:
    """The pose a frame is looked for at when its descriptor matched that of the keyframe at c2w_kf [4,4] under the
    shift (sx, sy) of the 16 x 12 grid: c2w_kf @ R_y(-a) @ R_x(+b), a = atan(sx (width / 16) / fx), b = atan(sy
    (height / 12) / fy) -- x right, y down, z forward, ``_step``'s rotations.  What the keyframe saw in cell (i, j) the
    frame sees in cell (i + sx, j + sy): sx cells to the right is a camera turned to the left about its y, sy cells
    down one tilted up about its x.  Composed in float64 and rounded to float32 once (no shift: the keyframe's pose
    bit for bit); on the host."""
    c2w = torch.as_tensor(c2w_kf).detach().cpu().double()
    a = math.degrees(math.atan(sx * (width / 16.0) / fx))
    b = math.degrees(math.atan(sy * (height / 12.0) / fy))
    return (c2w @ _step(1, rot_deg=-a) @ _step(0, rot_deg=b)).to(torch.float32)


def _default_factory(N, W, H, config, device, render_mode):
    from .graph_tracker import GraphTracker
    return GraphTracker(N, W, H, config, device=device, render_mode=render_mode)


class Localizer:
    """``reset(depth, rgb, c2w)`` with the first frame and its pose, then ``track(depth, rgb)`` per frame.
    depth [H,W] in metres, rgb [H,W,3] in 0..255 (as the dataset readers deliver them), poses 4x4 camera-to-world.
    ``tracker_factory(N, W, H, config, device, render_mode)`` returns what is driven through ``load_frame`` / ``run``
    (default: GraphTracker).  With ``config.rgb_lambda != 0`` every frame needs its image and the tracker renders
    "RGB+ED" whatever ``render_mode`` says.

    ``mode="frame"`` (default): frame to frame, as above.  ``mode="map"``: frame to map.  The Gaussians of every frame are
    the live points of a ``GaussianMap`` (``map_config``; ``map_factory(width, height, config, device)`` builds it), which
    are in the world already: ``reset`` fills it with every valid pixel of the first frame, and after every frame that
    is not lost the map is rendered once at the frame's estimate -- in the pair's frame, with the scales the tracker just
    used, by ``map_renderer(points, scales, Ks, c2w, height, width) -> (depth, alpha)`` (default: render_depth_alpha; the
    CPU tests use stand-ins for both) -- and the pixels it does not explain are appended (mapping.py).  The tracker is
    rebuilt when the live count changes.  ``map_config.view_guard_px``: the Gaussians of a frame are the live points in
    view from its start pose only (``GaussianMap.select_view``; ``LocalizeResult.tracked``), the tracker is keyed on
    their count, and ``LocalizeResult.view_violations`` says how many rows in reach of the view from the estimate they
    left out (above 0: the render is made from a selection at the estimate).  ``map_config.view_occlusion_rho``: of the
    rows in that view, those hidden behind nearer rows of the map are left out as well (``LocalizeResult.view_culled``),
    and the check at the estimate counts the rows visible from there: it also repairs an occlusion that no longer
    holds.  ``map_config.free_rho``: after the
    insertion (insert first, then remove: the insertion render is of the cloud that was tracked, and the rows just
    appended sit at their own pixel's observed depth and cannot go) the rows the frame sees through are removed,
    ``LocalizeResult.removed`` counts them and ``map_size`` is the count after the removal; the pixels behind a removed
    ghost are uncovered only now, so it is the next frame's insertion that fills the hole.  A lost frame removes
    nothing.  ``map_config.evict``: between the insertion render and the insertion the rows the frame observes from the
    estimate are stamped (``GaussianMap.observe``), and an insertion that does not fit evicts the least recently
    observed rows first (``LocalizeResult.evicted``; ``map_size`` never exceeds the capacity and the map is not
    ``full`` while enough rows are old enough to go); a lost frame stamps, evicts and inserts nothing.
    ``map_config.merge_voxel``: last of all -- after ``reset``'s insertion, and after the insertion and the free-space
    removal of every ``merge_every``-th call of ``track`` whose frame is not lost -- the rows that share a voxel are
    fused (``GaussianMap.merge``), ``LocalizeResult.merged`` counts the rows it removed (0 on the frames in between)
    and ``map_size`` is the count after it.  ``map_config.reloc``: first of all -- after ``run()``, before the band is
    checked or anything is rendered, stamped or inserted -- the estimate is scored against the map
    (``GaussianMap.score_poses``; ``LocalizeResult.tested`` / ``agree`` / ``front``) and accepted when the tracker
    recorded a minimum, at least ``reloc_min_tested`` rows were tested and ``agree >= reloc_min_agree * (agree +
    front)``.  If not, ``reloc_candidates`` around the start pose (and around the previous estimate, where the motion
    model made the two differ) are scored in one call and the one with the largest ``agree - front`` (the lowest index
    among equals) is tracked from, on a pair built at that pose; its estimate, if accepted, is the frame's
    (``relocalised``).  If it is not, or if the start that failed scored highest itself, the frame is ``lost`` -- which
    with this option means "not accepted" -- the better-scoring of the two estimates is handed on, and the map is left
    as it was.  ``steps`` counts both runs; ``best_step``, ``best_loss`` and ``init_c2w`` are those of the run that
    was kept.  ``map_config.keyframes``: ``reset`` keeps the first frame as keyframe 0 after its insertion, and every
    frame that is not lost is offered to ``GaussianMap.add_keyframe`` with its estimate after its insertion (and
    removal and merge: the descriptor reads the depth image only; ``LocalizeResult.keyframe``).  When the flow above
    ends with the frame lost -- an estimate rejected twice, or a grid whose winner is the failed start -- and the map
    has keyframes, the first ``place_top`` entries of ``GaussianMap.match_place`` give the bases ``place_base`` of one
    more ``reloc_candidates`` grid; one ``score_poses`` call scores it, the candidate with the largest ``agree -
    front`` (the lowest index among equals) is tracked from, and its estimate, if accepted, is the frame's
    (``relocalised``, and ``recognised`` is the slot of the winning base's keyframe).  If not, the frame stays lost, the
    map is left alone and the best-scoring estimate of all runs is handed on; ``steps`` counts every run.  With the
    option on and no frame rejected, poses, step counts and added rows are those of the run without it.
    ``map_config.refine``: after the insertion render and before ``observe`` and the insertion -- every live row is then
    an old one: the rows a frame appends sit at their own pixel's depth and must not count as observed again by that
    frame, and the render is of the cloud that was tracked -- the rows the frame observes again from the estimate are
    refined (``GaussianMap.refine``; ``LocalizeResult.refined`` counts them).  Their colours are refined with the
    frame's image only when the localizer is photometric (``rgb_lambda != 0``): without an image the frame's colours
    are a constant stand-in that must not bleach the stored ones.  A lost frame refines nothing.  Refinement at an
    estimated pose feeds a share 1 / (weight + 1) of that pose's error into the rows it moves.
    ``map_config.info``: for a frame that is not lost, one call of ``GaussianMap.pose_information`` at the frame's final
    estimate -- after the relocalisation flow, before the band is checked and before anything is rendered, refined,
    stamped or inserted -- fills ``LocalizeResult.cov`` / ``sigma_t`` / ``sigma_r`` / ``info_used`` / ``info_min_eig`` /
    ``weak``.  It reads the map and the depth image and writes neither: poses, steps, added rows and the map are bit
    for bit those of the run without the option.
    ``map_config.align``: before the pair is built, ``GaussianMap.align_pose`` aligns the motion model's start pose to
    the map against the frame's depth image.  A pose it moved (status CONVERGED or STEPPED) is scored beside the start
    in one ``score_poses`` call and taken when it confirms some row and its share agree / (agree + front) is at least
    the start's; a pose that is taken is what ``select_view``, ``build_pair`` and the tracker start from, it is
    ``init_c2w``, and the relocalisation grid, the insertion, refinement and information see it wherever they saw the
    start.  A pose that is not taken is dropped and the frame runs as without the option.  ``LocalizeResult.aligned`` /
    ``align_status`` / ``align_steps`` / ``align_from`` (the motion model's pose) / ``align_moved_t`` /
    ``align_moved_r_deg`` / ``align_scores`` say what happened.  Nothing in the map is written.  With the option off
    there is no call, and poses, step counts and the map are bit for bit those of the run without it.
    ``map_config.photo_scale`` (with ``info``, ``align`` or ``loop``): ``track`` makes the frame's intensity image once
    (``GaussianMap.intensity``; the frame then needs its ``rgb``) and hands it to every alignment, loop constraint and
    pose information of the frame, whose normal equations gain a photometric equation per used row
    (csrc/map_photo.hip); ``LocalizeResult.info_photo_used`` counts them.  A textured wall is then a frame that pins
    its pose down: not ``weak``, and with ``align_accept`` a direct one.  ``map_config.align_levels`` (with ``align``
    or ``loop``): ``track`` builds the frame's image pyramid once (``GaussianMap.pyramid``: depth and, with
    ``photo_scale``, intensity) and every alignment of the frame -- of the start pose, of ``reloc_align_top``'s
    candidates, of a loop constraint -- runs coarse to fine on it; ``LocalizeResult.align_level_steps`` holds the steps
    per level.  With the field at None every launch, buffer
    and number is as without it.
    ``map_config.photo_exposure`` (with ``photo_scale``): before any of that ``track`` estimates the frame's gain and
    offset against the map at its start pose (``GaussianMap.estimate_exposure``) and corrects the image
    (``apply_exposure``); the intensity image and the pyramid are made from the corrected image.  With ``align``, when
    the aligned start is taken the exposure is estimated once more there, and where that changes the pair the images
    are made again and the alignment is repeated from the aligned pose (``_realigned``).  For a frame that is
    not lost, before anything of it enters the map, the RAW image is corrected once more with an estimate at the
    frame's final pose: that image is what ``refine`` and ``insert_frame`` receive, and the estimate is what
    ``LocalizeResult.exposure_gain`` / ``exposure_offset`` / ``exposure_status`` / ``exposure_used`` report.  An
    estimate that is not OK corrects nothing.  The splat tracker's own pair keeps the raw image.  Off: every launch,
    buffer and number is as without the field.
    ``map_config.origins``: every appended pose is recorded with its odometry measurement, the float64 relative pose to
    the pose before it as it was appended (``reset`` clears the record, ``correct_trajectory`` leaves it alone), which
    is what ``add_loop`` builds its pose graph on.  ``map_config.loop``: for a frame that is not lost, before the pose
    information and before anything is rendered, refined, stamped, inserted or removed, ``track`` looks for a loop
    (``_try_loop`` has the steps; ``LocalizeResult.loop`` / ``loop_status`` / ``loop_old_tested`` / ``loop_anchor`` /
    ``loop_moved_t`` / ``loop_moved_r_deg`` / ``loop_correction``).  A frame that closes one has the corrected pose as
    its ``c2w``, and its insertion render is made from a new pair at that pose.  With no closure poses, step counts and
    the map are bit for bit those of the run without the option.  Everything else
    -- normalisation, the re-rendered query depth, the scales, the hand-over, ``best_c2w`` -- is the frame mode's."""

    def __init__(self, K: Tensor, width: int, height: int, config: TrackerConfig = TrackerConfig(),
                 normalize: bool = True, motion: str = "constant_velocity", device="cuda", render_mode: str = "ED",
                 tracker_factory: Optional[Callable] = None, mode: str = "frame",
                 map_config: Optional[MapConfig] = None, map_factory: Optional[Callable] = None,
                 map_renderer: Optional[Callable] = None):
        if motion not in MOTIONS:
            raise ValueError(f"unknown motion model {motion!r}: one of {MOTIONS}")
        if mode not in MODES:
            raise ValueError(f"unknown mode {mode!r}: one of {MODES}")
        self.device = torch.device(device)
        self.K = torch.as_tensor(K, dtype=torch.float32, device=self.device)
        self.W, self.H = int(width), int(height)
        self.cfg = config
        self.normalize = bool(normalize)
        self.motion = motion
        self.photo = config.rgb_lambda != 0.0
        self.render_mode = "RGB+ED" if self.photo else render_mode
        self._factory = tracker_factory if tracker_factory is not None else _default_factory
        self.tracker = None
        self._tracker_N = -1
        self._prev = None  # (camera-frame cloud [H*W,3], colours [H*W,3] in 0..1) of the last frame
        self._poses: List[Tensor] = []
        self.map_mode = mode == "map"
        self.map = None
        self._view_guard = None  # MapConfig.view_guard_px
        self._view_occlusion = None  # MapConfig.view_occlusion_rho
        self._free = False  # MapConfig.free_rho is set
        self._evict = False  # MapConfig.evict
        self._merge_every = 0  # MapConfig.merge_every when merge_voxel is set, else 0
        self._reloc = None  # the MapConfig when MapConfig.reloc is on
        self._min_tested = 0  # MapConfig.reloc_min_tested, or its default for this image size
        self._keyframes = False  # MapConfig.keyframes
        self._refine = False  # MapConfig.refine
        self._info = False  # MapConfig.info
        self._align = False  # MapConfig.align
        self._accept = None  # (align_accept_min_used, align_accept_min_eig) when MapConfig.align_accept is on
        self._photo_scale = None  # MapConfig.photo_scale
        self._photo_kw: dict = {}  # with it, inside track(): intensity=<the frame's intensity image>, for the map's calls
        self._align_levels = 0  # MapConfig.align_levels
        self._exposure = False  # MapConfig.photo_exposure
        # inside track(): _photo_kw and, with align_levels, levels= and pyramid=<the frame's>, for the map's alignments
        self._align_kw: dict = {}
        self._origins = False  # MapConfig.origins
        self._loop = None  # the MapConfig when MapConfig.loop is on
        self._loop_min_rows = 0  # MapConfig.loop_min_rows, or its default for this image size
        self._loop_weight, self._loop_by = 1e4, "index"  # MapConfig.loop_weight / loop_by (add_loop)
        self._odometry: List[np.ndarray] = []  # origins: float64 [4,4] per appended pose, inv(poses[-2]) poses[-1]
        self._loops: list = []  # the loop edges so far: (anchor, last, Z, weight)
        self._loop_last = 0  # the frame of the last attempt at a loop
        self.last_pose_graph = None  # the ``PoseGraphResult`` of the last add_loop
        self._tracked = 0  # calls of track since reset
        self.merged_at_reset = None  # merge_voxel: rows the merge after reset's insertion removed
        if self.map_mode:
            make = map_factory if map_factory is not None else GaussianMap
            map_config = map_config if map_config is not None else MapConfig()
            self.map = make(self.W, self.H, map_config, self.device)
            self._view_guard = map_config.view_guard_px
            self._view_occlusion = map_config.view_occlusion_rho
            self._free = map_config.free_rho is not None
            self._evict = bool(map_config.evict)
            self._merge_every = int(map_config.merge_every) if map_config.merge_voxel is not None else 0
            self._refine = bool(map_config.refine)
            self._info = bool(map_config.info)
            self._align = bool(map_config.align)
            self._photo_scale = map_config.photo_scale
            self._align_levels = int(map_config.align_levels)
            self._exposure = bool(map_config.photo_exposure)
            if map_config.align_accept:
                self._accept = (
                    (self.W * self.H) // 16 if map_config.align_accept_min_used is None else map_config.align_accept_min_used,
                    INFO_MIN_EIG if map_config.align_accept_min_eig is None else float(map_config.align_accept_min_eig))
            self._origins = bool(map_config.origins)
            self._loop_weight, self._loop_by = float(map_config.loop_weight), map_config.loop_by
            if map_config.loop:
                self._loop = map_config
                self._loop_min_rows = (map_config.loop_min_rows if map_config.loop_min_rows is not None
                                       else (self.W * self.H) // 8)
            if map_config.reloc:
                self._reloc = map_config
                self._min_tested = (map_config.reloc_min_tested if map_config.reloc_min_tested is not None
                                    else (self.W * self.H) // 16)
                self._keyframes = bool(map_config.keyframes)
        self._render_map = map_renderer if map_renderer is not None else render_depth_alpha

    def _frame(self, depth, rgb):
        depth = torch.as_tensor(depth, dtype=torch.float32, device=self.device)
        if depth.shape != (self.H, self.W):
            raise ValueError(f"depth is {tuple(depth.shape)}, the localizer was built for {(self.H, self.W)}")
        if rgb is None:
            if self.photo:
                raise ValueError(f"rgb_lambda = {self.cfg.rgb_lambda}: the photometric term needs every frame's image "
                                 "(rgb=)")
            rgb = torch.full((self.H, self.W, 3), 127.5, device=self.device)  # colours are not rendered in "ED"
        rgb = torch.as_tensor(rgb, dtype=torch.float32, device=self.device)[..., :3]
        return depth, rgb, depth_to_points(depth, self.K), (rgb / 255.0).reshape(-1, 3)

    def _map_pair(self, at: Tensor, frame):
        """The pair of a new frame (its clouds, images, placing and reference pose) and the map: all live points, or --
        ``view_guard_px`` -- those in view from the world pose ``at``, the image widened by the guard band (an empty
        selection: all of them)."""
        t_pts, t_col = self.map.points, self.map.point_colors
        culled = None
        if self._view_guard is not None:
            # (the keyword only with the option: without it the call is the one a map without the option gets)
            occlusion = {} if self._view_occlusion is None else dict(occlusion_rho=self._view_occlusion)
            v_pts, v_col, _, n = self.map.select_view(self.K, at, self._view_guard, self.cfg.gs.near_plane,
                                                      self.cfg.gs.far_plane, **occlusion)
            if n > 0:
                t_pts, t_col = v_pts, v_col
            if self._view_occlusion is not None:
                culled = self.map.last_view_culled
        pts, col, depth, rgb, placed, ref = frame
        d = build_pair(t_pts, t_col, pts, col, depth, rgb, placed, ref, self.K, self.normalize, t_placed=True)
        d.view_culled = culled  # travels with the pair: the frame reports the selection that was tracked
        return d

    def _map_render(self, d, scales: Tensor, c2w_n: Tensor):
        """What the pair's cloud shows from the pose ``c2w_n`` in the pair's frame (a rigid move of the world: depths in
        metres up to the pair's scale factor, which build_pair divides the query depth by as well)."""
        render, alphas = self._render_map(d.tar_points, scales, self.K.unsqueeze(0), c2w_n.unsqueeze(0), self.H, self.W)
        return render / d.pca_factor.reshape(()), alphas

    def _run_tracker(self, d, init: Tensor):
        """Steps 4 - 6 on the pair ``d`` from the world pose ``init``: (Gaussians tracked, their scales, the tracker's
        result, its minimum-loss pose in the pair's frame, that pose in the world)."""
        init_n = self._pair_pose(d, init)
        N = d.tar_points.shape[0]
        if self.tracker is None or self._tracker_N != N:
            self.tracker, self._tracker_N = self._factory(N, self.W, self.H, self.cfg, self.device, self.render_mode), N
        scales = init_gs_scales(d.tar_points)
        self.tracker.load_frame(d.tar_points, d.colors, scales, d.src_depth, init_n, d.src_c2w,
                                self.K, pixels=d.pixels if self.photo else None)
        res = self.tracker.run()
        best = res.best_c2w.to(self.device)
        est = denormalize_camera(d.norm_T, best) if d.norm_T is not None else best.clone()
        return N, scales, res, best, est

    def _verdict(self, depth: Tensor, c2w: Tensor):
        """(tested, agree, front), Python ints: the map's rows that the depth frame judges from the world pose c2w."""
        return tuple(int(c) for c in self.map.score_poses(depth, self.K, [c2w], self.cfg.gs.near_plane)[0])

    def _accepted(self, res, verdict, direct: bool = False) -> bool:
        """reloc: the tracker recorded a minimum (direct: it did not run, the map's verdict decides alone), enough rows
        were tested, and of those the frame judges against its own surface -- in front of it or on it -- at least
        ``reloc_min_agree`` are on it."""
        tested, agree, front = verdict
        return ((direct or res.best_step != -1) and tested >= self._min_tested
                and agree >= self._reloc.reloc_min_agree * (agree + front))

    def _pair_pose(self, d, c2w: Tensor) -> Tensor:
        """The world pose c2w in the frame of the pair ``d``."""
        return transform_cameras(d.norm_T, c2w.unsqueeze(0))[0].squeeze(0) if d.norm_T is not None else c2w

    def _direct_run(self, d, est: Tensor):
        """What ``_run_tracker`` returns, for a frame whose estimate is the aligned pose ``est`` and whose pair ``d`` was
        built there: no step, no minimum, no loss."""
        at = self._pair_pose(d, est)
        res = TrackResult(best_loss=None, steps=0, final_c2w=at, best_c2w=at, best_step=-1)
        return d.tar_points.shape[0], init_gs_scales(d.tar_points), res, at, est.clone()

    def _share_rule(self, start, aligned) -> bool:
        """An aligned pose against the pose it started from, by their (tested, agree, front): the aligned pose confirms
        some row, and its share of agreeing rows is at least the start's (``_aligned_start``)."""
        (_, agree_s, front_s), (_, agree_a, front_a) = start, aligned
        return agree_a > 0 and agree_a * front_s >= agree_s * front_a

    def _direct_reason(self, al, taken: bool) -> Optional[str]:
        """align_accept: None when the alignment ``al`` (of ``GaussianMap.align_poses``), which the share rule took or
        did not, may be the frame's estimate; otherwise the first rule that failed."""
        min_used, min_eig = self._accept
        if al.status != "CONVERGED":
            return "status"
        if not al.closed:
            return "open"
        if not taken:
            return "share"
        if al.final.used < min_used:
            return "used"
        if al.final.weak(min_eig):
            return "weak"
        return None

    def _aligned_start(self, depth: Tensor, init: Tensor):
        """align: the motion model's pose aligned to the map (``GaussianMap.align_pose``), and taken when the alignment
        moved it (status CONVERGED or STEPPED) and the map scores it no worse -- one ``score_poses`` call on the two:
        the aligned pose confirms some row, and of the rows it judges against the frame's own surface (those that
        agree and those in front) the share that agrees is at least the start's, agree_a * front_s >= agree_s * front_a
        in integers.  The share, the quantity ``reloc`` accepts an estimate by, and not the difference agree - front:
        a camera that moves loses rows over the image's edge, and the difference counts every one of them against
        the pose that follows the motion (NOTES.md, "Pose alignment").  Returns (the ``LocalizeResult`` fields aligned,
        align_status, align_steps, align_from, align_moved_t, align_moved_r_deg, align_scores; the pose to start
        from; align_accept: None when that pose may be the frame's estimate, else ``_direct_reason``'s word -- None
        with the option off).  With ``align_levels`` the alignment runs coarse to fine on the frame's pyramid, and the
        fields gain the steps per level."""
        near = self.cfg.gs.near_plane
        if self._accept is None:
            al = self.map.align_pose(depth, self.K, init, near, **self._align_kw)
        else:  # the same pose bit for bit, and the sums at it
            al = self.map.align_poses(depth, self.K, [init], near, **self._align_kw)[0]
        taken, moved_t, moved_r, scores = False, 0.0, 0.0, None
        if al.status in ("CONVERGED", "STEPPED"):
            to = al.c2w.to(self.device)
            moved_t, moved_r = float(calculate_translation_error(to, init)), float(calculate_rotation_error(to, init))
            scores = tuple(tuple(int(c) for c in s) for s in self.map.score_poses(depth, self.K, [init, to], near))
            taken = self._share_rule(*scores)
        reason = None if self._accept is None else self._direct_reason(al, taken)
        return (taken, al.status, al.steps, init, moved_t, moved_r, scores, al.level_steps), (to if taken else init), reason

    def _frame_images(self, depth: Tensor, rgb: Optional[Tensor]) -> None:
        """What the map's calls of this frame read: the intensity image of rgb (None: no photometric term) and, with
        ``align_levels``, the frame's pyramid, every alignment of the frame starts at its coarsest level."""
        self._photo_kw = {} if rgb is None else dict(intensity=self.map.intensity(rgb))
        self._align_kw = self._photo_kw
        if self._align_levels > 0:
            self._align_kw = dict(self._photo_kw, levels=self._align_levels, pyramid=self.map.pyramid(
                depth, self._align_levels, intensity=self._photo_kw.get("intensity")))

    def _realigned(self, depth: Tensor, rgb: Tensor, exposure, alignment, init: Tensor, reason):
        """photo_exposure, after an aligned start was taken: the exposure is estimated once more, at the aligned pose.
        The estimate reads every row's NEAREST pixel, so it depends on the pose through which pixel a row rounds to: a
        start a fraction of a pixel off makes the frame's intensity a noisy regressor and the gain comes out 0.15 ..
        0.25 % low, which costs the alignment a factor of three (NOTES.md, "Exposure compensation").  Where the second
        estimate is OK and another pair than the first, the frame's images are made again from it and the alignment is
        repeated from the aligned pose; its verdict (taken or not, ``align_accept``'s reason) is the frame's, the
        steps add up, and ``align_from`` / ``align_moved_*`` stay relative to the motion model's pose.  Returns
        (exposure, the ``_aligned_start`` fields, the pose to start from, the reason)."""
        again, seen = self._corrected(depth, rgb, init)
        if not again.ok or (exposure.ok and (again.gain, again.offset) == (exposure.gain, exposure.offset)):
            return exposure, alignment, init, reason
        self._frame_images(depth, seen)
        second, to, why = self._aligned_start(depth, init)
        start = alignment[3]
        moved_t, moved_r = float(calculate_translation_error(to, start)), float(calculate_rotation_error(to, start))
        levels = None if second[7] is None else [a + b for a, b in zip(alignment[7], second[7])]
        fields = (True, second[1], alignment[2] + second[2], start, moved_t, moved_r,
                  alignment[6] if second[6] is None else second[6], levels)
        return again, fields, to, why

    def _corrected(self, depth: Tensor, rgb: Tensor, c2w: Tensor):
        """(the ``Exposure`` of the raw image rgb against the map at c2w, the image it corrects to: rgb itself when the
        estimate is not OK)."""
        exposure = self.map.estimate_exposure(depth, self.K, c2w, self.cfg.gs.near_plane, rgb=rgb)
        return exposure, self.map.apply_exposure(rgb) if exposure.ok else rgb

    @staticmethod
    def _report_information(out: LocalizeResult, info) -> None:
        """The fields of a frame's result that ``MapConfig.info`` fills, from its ``PoseInformation``."""
        out.info_used, out.info_min_eig, out.weak = info.used, float(info.eigenvalues[0]), info.weak()
        out.cov = info.covariance()
        if out.cov is not None:
            out.sigma_t = math.sqrt(float(out.cov[3:, 3:].trace()))
            out.sigma_r = math.degrees(math.sqrt(float(out.cov[:3, :3].trace())))

    @property
    def trajectory(self) -> Tensor:
        """[n,4,4] the world poses so far, frame 0 included."""
        return torch.stack(self._poses) if self._poses else torch.zeros(0, 4, 4, device=self.device)

    def reset(self, depth, rgb=None, c2w: Optional[Tensor] = None) -> None:
        """The first frame and its pose (identity by default); forgets the trajectory so far."""
        depth, rgb, pts, col = self._frame(depth, rgb)
        pose = torch.eye(4) if c2w is None else torch.as_tensor(c2w, dtype=torch.float32)
        self._prev = (pts, col)
        self._poses = [pose.to(self.device).clone()]
        self._odometry, self._loops, self._loop_last, self.last_pose_graph = [], [], 0, None
        self._photo_kw, self._align_kw = {}, {}
        if self.map_mode:
            self.map.clear()
            first = dict(origin=0) if self._origins else {}  # the index of the frame's pose in the trajectory
            self.map.insert_frame(depth, rgb, self.K, self._poses[0], **first)  # no render yet: every valid pixel
            self._tracked = 0
            if self._merge_every:
                self.merged_at_reset = self.map.merge()[0]
            if self._keyframes:
                self.map.add_keyframe(depth, self._poses[0], **first)  # keyframe 0: clear() has forgotten the others

    def _retry(self, depth: Tensor, frame, bases, kept, failed_start: bool = False):
        """One more run for a frame whose estimate the map rejected.  The ``reloc_candidates`` around the bases are scored
        in one call; the one with the largest ``agree - front`` (the lowest index among equals) is tracked from, on a
        pair built at that pose, and the estimate is held against the map.  kept: (run as ``_run_tracker`` returns it,
        pair, start pose, verdict) of the run kept so far.  Returns (that candidate's index, accepted, the run's steps,
        the state to keep now, (candidates replaced by their alignment -- None with reloc_align_top at 0 --, the run
        was a direct one)) -- or None when failed_start says that candidate 0 is the start that has just failed, and
        it scores highest.
        reloc_align_top: the candidates with the largest margins, that many (the lowest index among equals), are
        aligned in one ``align_poses`` call and the aligned poses scored in one more; an alignment that moved and that
        passes ``_share_rule`` against its own candidate takes the candidate's place and margin before the winner is
        chosen.  With align_accept a winner that is such an alignment and passes ``_direct_reason`` is the estimate
        without a tracking, when the map accepts it."""
        cfg, near = self._reloc, self.cfg.gs.near_plane
        cands = reloc_candidates(bases, cfg.reloc_rot_deg, cfg.reloc_trans, cfg.reloc_levels).to(self.device)
        scores = self.map.score_poses(depth, self.K, cands, near)
        margins = [int(s[1]) - int(s[2]) for s in scores]
        aligned = {}  # candidate -> the alignment that took its place
        if cfg.reloc_align_top > 0:
            top = sorted(range(len(margins)), key=lambda i: (-margins[i], i))[: cfg.reloc_align_top]
            als = self.map.align_poses(depth, self.K, [cands[i] for i in top], near, **self._align_kw)
            tos = [al.c2w.to(self.device) for al in als]
            cands = cands.clone()
            for i, al, to, sc in zip(top, als, tos, self.map.score_poses(depth, self.K, tos, near)):
                if al.moved and self._share_rule(tuple(int(c) for c in scores[i]), tuple(int(c) for c in sc)):
                    cands[i], margins[i], aligned[i] = to.to(cands.dtype), int(sc[1]) - int(sc[2]), al
        replaced = len(aligned) if cfg.reloc_align_top > 0 else None
        winner = margins.index(max(margins))  # the lowest index among equals
        if failed_start and winner == 0 and 0 not in aligned:
            return None
        pair = self._map_pair(cands[winner], frame)
        run, direct = None, False
        if self._accept is not None and winner in aligned and self._direct_reason(aligned[winner], True) is None:
            run = self._direct_run(pair, cands[winner])
            verdict = self._verdict(depth, run[4])
            direct = self._accepted(run[2], verdict, direct=True)
        if not direct:
            run = self._run_tracker(pair, cands[winner])
            verdict = self._verdict(depth, run[4])
        accepted = direct or self._accepted(run[2], verdict)
        if accepted or verdict[1] - verdict[2] > kept[3][1] - kept[3][2]:  # better-scoring, rejected: still handed on
            kept = (run, pair, cands[winner], verdict)
        return winner, accepted, run[2].steps, kept, (replaced, direct)

    def _recognise(self, depth: Tensor, frame, kept):
        """Place recognition for a frame that the grid around its start poses has left lost: ``_retry`` around the turned
        poses of the best-matching keyframes, with the keyframe slot of the winning base in place of the winner; None
        when no keyframe has an admissible match."""
        ranked = self.map.match_place(depth)[: self._reloc.place_top]
        if not ranked:
            return None
        poses = self.map.keyframe_poses
        fx, fy = float(self.K[0, 0]), float(self.K[1, 1])
        bases = [place_base(poses[slot], sx, sy, self.W, self.H, fx, fy) for slot, sx, sy, _, _ in ranked]
        winner, *rest = self._retry(depth, frame, bases, kept)
        return (ranked[winner // (1 + 12 * self._reloc.reloc_levels)][0], *rest)

    def track(self, depth, rgb=None, gt_c2w: Optional[Tensor] = None) -> LocalizeResult:
        try:
            return self._track_frame(depth, rgb, gt_c2w)
        finally:
            # the intensity image and the pyramid are the frame's: nothing outside its track() may read them
            self._photo_kw, self._align_kw = {}, {}

    @torch.no_grad()
    def _track_frame(self, depth, rgb, gt_c2w: Optional[Tensor]) -> LocalizeResult:
        if self._prev is None:
            raise RuntimeError("Localizer.track before reset(): the first frame comes with its pose")
        if self._photo_scale is not None and rgb is None:
            raise ValueError(f"photo_scale = {self._photo_scale}: the photometric term of the map's normal equations "
                             "needs every frame's image (rgb=)")
        depth, rgb, pts, col = self._frame(depth, rgb)
        # the frame's intensity image, once: every alignment, loop constraint and pose information of the frame reads it
        exposure = None
        if self._exposure and self.map.n_live > 0:
            # the frame's exposure against the map, at the pose the frame starts from: what every alignment, loop
            # constraint and pose information of the frame reads is the corrected image's intensity
            start = self._poses[-1] if self.motion == "hold" or len(self._poses) < 2 else predict_pose(
                self._poses[-2], self._poses[-1])
            exposure, seen = self._corrected(depth, rgb, start)
            self._frame_images(depth, seen)
        else:
            self._frame_images(depth, None if self._photo_scale is None else rgb)
        placed = self._poses[-1]
        if self.motion == "hold" or len(self._poses) < 2:
            init = placed
        else:
            init = predict_pose(self._poses[-2], placed)
        gt = None if gt_c2w is None else torch.as_tensor(gt_c2w, dtype=torch.float32, device=self.device)
        alignment, direct, reason = None, None, None
        # the pair's reference pose is the tracker's error read-out only: without ground truth, the starting pose
        if self.map_mode:
            if self.map.n_live == 0:
                raise RuntimeError("Localizer.track: the map is empty (the first frame had no valid depth)")
            if self._align:
                alignment, init, reason = self._aligned_start(depth, init)
                if exposure is not None and alignment[0]:
                    exposure, alignment, init, reason = self._realigned(depth, rgb, exposure, alignment, init, reason)
                direct = None if self._accept is None else reason is None
            frame = (pts, col, depth, rgb, placed, gt if gt is not None else init)
            d = self._map_pair(init, frame)
        else:
            d = build_pair(self._prev[0], self._prev[1], pts, col, depth, rgb, placed, gt if gt is not None else init,
                           self.K, self.normalize)
        run, verdict = None, None
        if direct:
            # the aligned pose is the estimate, on the pair built there.  reloc holds it against the map as any estimate;
            # one it rejects is dropped, and the frame runs from the motion model's start as without the options
            run = self._direct_run(d, init)
            if self._reloc is not None:
                verdict = self._verdict(depth, run[4])
                if not self._accepted(run[2], verdict, direct=True):
                    run, verdict, direct, reason, init = None, None, False, "rejected", alignment[3]
                    frame = (pts, col, depth, rgb, placed, gt if gt is not None else init)
                    d = self._map_pair(init, frame)
        N, scales, res, best, est = run if run is not None else self._run_tracker(d, init)
        steps, lost, relocalised, recognised, reloc_aligned = res.steps, res.best_step == -1 and not direct, None, None, None
        if self._reloc is not None:
            # before anything touches the map: does it confirm the estimate?  If not, the best-scoring pose of a grid
            # around the start poses is tracked from once more; an estimate the map still rejects is a lost frame's
            verdict, relocalised = self._verdict(depth, est) if verdict is None else verdict, False
            lost = not self._accepted(res, verdict, direct=bool(direct))
            kept = ((N, scales, res, best, est), d, init, verdict)
            if lost:
                again = self._retry(depth, frame, [init] if torch.equal(placed, init) else [init, placed], kept, True)
                if again is not None:
                    _, relocalised, more, kept, (reloc_aligned, took) = again
                    steps, lost = steps + more, not relocalised
                    if took:
                        direct, reason = True, None
            if self._keyframes:
                recognised = -1
                found = self._recognise(depth, frame, kept) if lost and self.map.n_keyframes > 0 else None
                if found is not None:
                    slot, accepted, more, kept, (reloc_aligned, took) = found
                    steps += more
                    if accepted:
                        lost, relocalised, recognised = False, True, slot
                        if took:
                            direct, reason = True, None
            (N, scales, res, best, est), d, init, verdict = kept
        self._prev = (pts, col)
        self._poses.append(est)
        if self._origins:
            # the odometry measurement, taken when the pose is appended: what was tracked, whatever is corrected later
            a, b = (p.detach().cpu().double().numpy() for p in self._poses[-2:])
            self._odometry.append(np.linalg.inv(a) @ b)
        out = LocalizeResult(c2w=est, init_c2w=init, steps=steps, best_step=res.best_step, best_loss=res.best_loss,
                             lost=lost)
        if verdict is not None:
            out.relocalised, (out.tested, out.agree, out.front) = relocalised, verdict
            out.recognised, out.reloc_aligned = recognised, reloc_aligned
        if alignment is not None:
            (out.aligned, out.align_status, out.align_steps, out.align_from, out.align_moved_t,
             out.align_moved_r_deg, out.align_scores, out.align_level_steps) = alignment
            out.direct, out.direct_reason = direct, reason
        if self.map_mode:
            out.added, out.tracked = 0, N
            out.view_culled = getattr(d, "view_culled", None)
            out.removed = 0 if self._free else None
            out.evicted = 0 if self._evict else None
            out.merged = 0 if self._merge_every else None
            out.refined = 0 if self._refine else None
            self._tracked += 1
            if self._loop is not None:
                out.loop = False
            if not out.lost:  # a lost frame's pose is a guess: it adds nothing
                if self._loop is not None:
                    # before anything touches the map: at a drifted pose the free-space rule would take correct old
                    # rows for ghosts, and the rows this frame appends should land where the closed loop puts them
                    self._try_loop(out, depth, est)
                    if out.loop:
                        est = out.c2w = self._poses[-1]
                if self._info:
                    # the frame's final estimate against the map as it was tracked: before anything below touches it
                    info = self.map.pose_information(depth, self.K, est, self.cfg.gs.near_plane, **self._photo_kw)
                    self._report_information(out, info)
                    if self._photo_scale is not None:
                        out.info_photo_used = info.photo_used
                if self._exposure:
                    # before anything of the frame enters the map: the raw image, corrected by the estimate at the
                    # frame's final pose -- the map stays in the exposure of its first frame
                    exposure, rgb = self._corrected(depth, rgb, est)
                at = best
                if out.loop:
                    # the rows have moved and the estimate with them: the insertion render is made from a new pair at
                    # the corrected pose (no second tracking), as below where the band did not hold
                    d = self._map_pair(est, frame)
                    scales = init_gs_scales(d.tar_points)
                    at = self._pair_pose(d, est)
                if self._view_guard is not None:
                    # the band is checked against the estimate, not assumed: rows that reach into the view from there
                    # and were not tracked would render as an empty border, and insert_frame would add them a second
                    # time.  Then the insertion render is made from a selection at the estimate (no second tracking)
                    out.view_violations = self.map.view_violations(self.K, est, self.cfg.gs.near_plane,
                                                                   self.cfg.gs.far_plane)
                    if out.view_violations > 0:
                        d = self._map_pair(est, frame)
                        scales = init_gs_scales(d.tar_points)
                        at = self._pair_pose(d, est)
                render, alphas = self._map_render(d, scales, at)
                if self._refine:
                    # after the render, before the insertion: every live row is an old one, and the render above is of
                    # the cloud that was tracked
                    out.refined = self.map.refine(depth, rgb if self.photo else None, self.K, est,
                                                  self.cfg.gs.near_plane)
                if self._evict:
                    # stamp before the insertion: what this frame observes must not make room for its own rows
                    self.map.observe(depth, self.K, est, self.cfg.gs.near_plane, self.cfg.gs.far_plane)
                index = dict(origin=len(self._poses) - 1) if self._origins else {}  # of est in the trajectory
                _, out.added = self.map.insert_frame(depth, rgb, self.K, est, render, alphas, **index)
                if self._evict:
                    out.evicted = self.map.last_evicted
                if self._free:
                    # insert first, then remove: the insertion render was made from the cloud that was tracked, and
                    # the rows just appended sit at their own pixel's observed depth
                    out.removed, _ = self.map.remove_seen_through(depth, self.K, est, self.cfg.gs.near_plane)
                if self._merge_every and self._tracked % self._merge_every == 0:
                    out.merged, _ = self.map.merge()
                if self._keyframes:
                    # after the frame is done: the descriptor reads the depth image only, nothing above depends on it
                    out.keyframe = self.map.add_keyframe(depth, est, **index)
            out.map_size = self.map.n_live
            if exposure is not None:
                ok = exposure.ok
                out.exposure_gain, out.exposure_offset = (exposure.gain, exposure.offset) if ok else (1.0, 0.0)
                out.exposure_status, out.exposure_used = exposure.status, exposure.used
        if gt is not None:
            out.eT, out.eR = calculate_translation_error(est, gt), calculate_rotation_error(est, gt)
        return out

    # ---- trajectory correction (MapConfig.origins) ------------------------------------------------------------------
    def _old_poses(self, what: str) -> np.ndarray:
        if not self.map_mode or not self._origins:
            raise RuntimeError(f"Localizer.{what}: needs mode='map' and MapConfig.origins=True -- without the frame every "
                               "row came from there is nothing a corrected trajectory could move")
        if not self._poses:
            raise RuntimeError(f"Localizer.{what} before reset(): there is no trajectory yet")
        return torch.stack(self._poses).detach().cpu().double().numpy()

    @torch.no_grad()
    def correct_trajectory(self, new_poses) -> TrajectoryCorrection:
        """Replaces the trajectory by new_poses [n,4,4], one pose per pose so far, and moves the map with it: the rows
        that frame k appended, and the keyframe made of frame k, move by D_k = new_k old_k^-1 (float64;
        ``GaussianMap.correct``).  A pose that is given back as it is has the identity as its D_k, and its rows keep
        every bit.  The next frame's motion model reads the corrected poses."""
        old = self._old_poses("correct_trajectory")
        new = torch.as_tensor(new_poses).detach().cpu().double().numpy()
        if new.shape != old.shape:
            raise ValueError(f"new_poses are {new.shape}, the trajectory is {old.shape}: one pose per pose so far")
        if not np.isfinite(new).all():
            raise ValueError("new_poses: some entry is not finite")
        D = np.tile(np.eye(4), (len(old), 1, 1))
        for k in range(len(old)):
            if not np.array_equal(new[k], old[k]):
                D[k] = new[k] @ np.linalg.inv(old[k])
                D[k, 3] = (0.0, 0.0, 0.0, 1.0)
        moved, outside = self.map.correct(D)
        self._poses = [torch.from_numpy(p.astype(np.float32)).to(self.device) for p in new]
        changed = [k for k in range(len(D)) if not np.array_equal(D[k], np.eye(4))]
        cos = np.clip((np.trace(D[:, :3, :3], axis1=1, axis2=2) - 1.0) / 2.0, -1.0, 1.0)
        return TrajectoryCorrection(moved=moved, outside=outside, frames=len(changed),
                                    max_trans=float(np.linalg.norm(D[:, :3, 3], axis=1).max()),
                                    max_rot_deg=float(np.degrees(np.arccos(cos)).max()))

    @torch.no_grad()
    def add_loop(self, anchor: int, last: int, c2w_last, weight: Optional[float] = None) -> TrajectoryCorrection:
        """One more loop constraint for the pose graph, the counterpart of ``close_loop`` that several constraints can
        share a trajectory through: frame ``last`` stood at c2w_last [4,4] as seen from frame ``anchor`` where it is now
        -- the edge (anchor, last, pose(anchor)^-1 c2w_last, weight; None: ``MapConfig.loop_weight``) joins the edges
        kept since ``reset``.  The graph of the tracked odometry (the relative pose of every appended pose to the one
        before, as it was appended) and all loop edges is optimised from the current trajectory
        (``optimise_pose_graph``, odometry weights by ``MapConfig.loop_by``), the frames up to the smallest anchor of
        any edge held, and the trajectory and the map are corrected (``correct_trajectory``).  ``last_pose_graph`` keeps
        the ``PoseGraphResult``.  An edge the graph refuses is not kept."""
        old = self._old_poses("add_loop")
        target = torch.as_tensor(c2w_last).detach().cpu().double().numpy()
        if target.shape != (4, 4):
            raise ValueError(f"c2w_last is {target.shape}, not (4, 4)")
        for name, v in (("anchor", anchor), ("last", last)):
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not 0 <= v < len(old):
                raise ValueError(f"{name} {v!r}: an index into the {len(old)} poses")
        if anchor >= last:
            raise ValueError(f"anchor {anchor} is not before last {last}")
        edge = (int(anchor), int(last), np.linalg.inv(old[anchor]) @ target,
                float(self._loop_weight if weight is None else weight))
        loops = self._loops + [edge]
        result = optimise_pose_graph(old, self._odometry, loops, min(e[0] for e in loops), by=self._loop_by)
        self._loops, self.last_pose_graph = loops, result
        return self.correct_trajectory(result.poses)

    def _try_loop(self, out: LocalizeResult, depth: Tensor, est: Tensor) -> None:
        """MapConfig.loop: the policy of one frame that is not lost, whose estimate ``est`` is the last pose of the
        trajectory and whose rows are not in the map yet; fills the ``loop`` fields of its result.
        (a) ``waiting``: fewer than ``loop_every`` frames since the last attempt.  (b) The covisibility at the estimate;
        the old frames are those up to n - ``loop_min_gap``: ``few_rows`` when they are tested fewer than
        ``loop_min_rows`` times.  (c) ``loop_constraint`` against the rows of the old frames: ``not_converged`` unless the
        alignment moved and CONVERGED.  (d) ``rejected`` unless the aligned pose agrees with at least ``loop_min_agree`` of
        the old rows it tests and with no smaller a share than the estimate (in integers).  (e) ``small``: the move is
        below ``loop_min_trans`` and below ``loop_min_rot_deg``.  (f) ``closed``: the anchor is the old frame with the
        most rows agreeing from the aligned pose (the lowest index among equals), and ``add_loop`` does the rest."""
        cfg, near, n = self._loop, self.cfg.gs.near_plane, len(self._poses) - 1
        if n - self._loop_last < cfg.loop_every:
            out.loop_status = "waiting"
            return
        self._loop_last = n
        upto = n - cfg.loop_min_gap  # the last old frame
        out.loop_old_tested = 0
        if upto >= 0:
            out.loop_old_tested = int(self.map.covisibility(depth, self.K, est, near, n_frames=n)[:upto + 1, 0].sum())
        if out.loop_old_tested < self._loop_min_rows:
            out.loop_status = "few_rows"
            return
        c = self.map.loop_constraint(depth, self.K, est, upto, near, **self._align_kw)
        if not (c.alignment.moved and c.alignment.status == "CONVERGED"):
            out.loop_status = "not_converged"
            return
        (tested_e, agree_e, _), (tested_a, agree_a, _) = (tuple(int(v) for v in s) for s in (c.scores, c.aligned_scores))
        if not (tested_a > 0 and agree_a >= cfg.loop_min_agree * tested_a and agree_a * tested_e >= agree_e * tested_a):
            out.loop_status = "rejected"
            return
        aligned = c.alignment.c2w.to(self.device)
        out.loop_moved_t = float(calculate_translation_error(aligned, est))
        out.loop_moved_r_deg = float(calculate_rotation_error(aligned, est))
        if out.loop_moved_t < cfg.loop_min_trans and out.loop_moved_r_deg < cfg.loop_min_rot_deg:
            out.loop_status = "small"
            return
        agree = self.map.covisibility(depth, self.K, aligned, near, n_frames=n)[:upto + 1, 1]
        out.loop_anchor = int(np.argmax(agree))  # the lowest index among equals
        out.loop_correction = self.add_loop(out.loop_anchor, n, aligned)
        out.loop, out.loop_status = True, "closed"

    @torch.no_grad()
    def close_loop(self, first: int, last: int, c2w_last, by: str = "path") -> TrajectoryCorrection:
        """One loop constraint: frame ``last`` of the trajectory really stood at c2w_last [4,4] (from
        ``GaussianMap.loop_constraint``, a place recogniser, a pose graph), and frame ``first`` and the frames before it
        are right as they are.  The correction delta = c2w_last c2w_old(last)^-1 is spread over the frames in between
        (``spread_correction``: by the camera's path length, or by="index"), the frames after ``last`` move with it,
        and the trajectory and the map are corrected (``correct_trajectory``)."""
        old = self._old_poses("close_loop")
        target = torch.as_tensor(c2w_last).detach().cpu().double().numpy()
        if target.shape != (4, 4):
            raise ValueError(f"c2w_last is {target.shape}, not (4, 4)")
        if isinstance(last, bool) or not isinstance(last, (int, np.integer)) or not 0 <= last < len(old):
            raise ValueError(f"last {last!r}: an index into the {len(old)} poses")
        # the pose the frame already has is no correction at all, not one of the size of a rounding error
        delta = np.eye(4) if np.array_equal(target, old[last]) else target @ np.linalg.inv(old[last])
        D = spread_correction(old, first, last, delta, by)
        return self.correct_trajectory(D @ old)
