"""A Gaussian map grown on the device: the persistent point cloud ``Localizer(mode="map")`` tracks frames against.

The map is means and colours in the world, ``capacity`` preallocated rows of which the first ``n_live`` are live.  A frame
adds the back-projection of the pixels the map does not explain yet (csrc/map.hip): pixels with a valid depth where the
map's render at the frame's pose has alpha below ``alpha_min`` (not covered) or shows a surface more than ``depth_rho``
behind the observed one (something stands in front).  Pixels without depth never enter.  Scales are not stored: they are
the reference's construction (``init_gs_scales``) on the cloud that is tracked.

The selection, the raster-order compaction, the back-projection and the append are two entry points and four launches;
the host reads the two counters back once per frame.  There is no CPU path.

The local map (``MapConfig.view_guard_px``, csrc/map_view.hip): ``select_view`` compacts the live rows in view from a
pose, the image widened by a guard band, in map order into working buffers -- what ``Localizer(mode="map")`` then
tracks instead of every live row -- and ``view_violations`` counts the rows in reach of the view from another pose that
this selection left out.  Two more entry points; each of the two calls reads its counters back once.

Occlusion culling (``MapConfig.view_occlusion_rho``, csrc/map_occl.hip): ``select_view(occlusion_rho=)`` first splats the
rows in the band into a coarse z-buffer of the map's own nearest depths and leaves out the rows that every cell around
their own hides; ``view_violations`` then counts the rows VISIBLE from the other pose that were left out, and
``view_depth`` returns the buffer.  Two entry points in front of the local map's gather; still one read-back per call.

Free space (``MapConfig.free_rho``, csrc/map_free.hip): ``remove_seen_through`` removes the live rows a depth frame sees
through -- rows that project into the image and lie more than ``free_rho`` in front of everything the frame observes in
a window of ``free_window_px`` pixels around their pixel -- and compacts the survivors, in map order, into a spare pair
of buffers that then becomes the map.  One more entry point and the local map's gather; one read-back.

A bounded map (``MapConfig.evict``, csrc/map_evict.hip): every row carries the index of the last frame that observed it
(``stamps``; ``observe`` stamps the rows a frame sees where it expects them, the rows a frame appends get its index), and
when a frame's new rows do not fit ``insert_frame`` first evicts exactly as many rows as are short -- the least recently
observed first, in map order among equals (``evict``) -- into the same spare buffers.  Only such a frame reads the
selection's count back before the append; a frame with room to spare keeps its single synchronisation.

A map with a resolution (``MapConfig.merge_voxel``, csrc/map_merge.hip): ``merge`` fuses the live rows that share a
voxel of that side into one row at the first of them, in integer arithmetic that does not depend on the order of the
rows, and compacts the rows that stay, in map order, into the same spare buffers.  Two more entry points, the local
map's gather and the stamps' gather; one read-back.

Pose scores (``MapConfig.reloc``, csrc/map_score.hip): ``score_poses`` counts, for each of up to 64 poses at once, the
live rows a depth frame tests, those it confirms (within ``depth_rho`` of the depth their own pixel observes) and those
it sees through (in front of that depth) -- integer counts, the same on every run -- which is what
``Localizer(mode="map")`` accepts an estimate by and chooses a new start by when it does not (localizer.py).  It changes
nothing in the map.  One more entry point; one read-back.

Place recognition (``MapConfig.keyframes``, csrc/map_place.hip): the map remembers what the frames that built it looked
like -- ``add_keyframe`` keeps the pose of a frame that lies far enough from every stored one and a 16 x 12 integer
descriptor of its depth image (``describe``), in a ring of ``keyframe_max`` -- and ``match_place`` holds a frame's
descriptor against all of them under 15 small shifts of the grid and ranks the keyframes it resembles, which is where
``Localizer(mode="map")`` looks for a frame that the relocalisation above has given up on.  Two more entry points;
``match_place`` reads back once, ``add_keyframe`` never.

Refinement (``MapConfig.refine``, csrc/map_refine.hip): a row is written from one pixel of one depth frame and keeps that
pixel's error; with the option every row carries a weight (``weights``, 1 for a row just appended), and ``refine`` moves
the live rows a depth frame observes again -- every one of the four pixels around their projection shows their depth
within ``refine_rho`` -- along their own ray to the running mean of the depths observed there (the four pixels' inverse
depths blended at the row's position), blends their colours likewise and raises their weight up to
``refine_max_weight``.  One more entry point; one read-back.  The weights follow their rows through every removal as
the stamps do.

Pose information (``MapConfig.info``, csrc/map_info.hip): ``pose_information`` sums the point-to-plane normal equations
of a pose over the live rows that agree with a depth frame on a planar patch -- the 6 x 6 information matrix, the
gradient and the residual sum, in fixed point, the same integers on every run -- and ``PoseInformation`` makes the
covariance of the pose, the verdict ``weak`` and, for the tests, the Gauss-Newton step of them (``apply_twist``).  It
changes nothing in the map.  One more entry point; one read-back.

Pose alignment (``MapConfig.align``, csrc/map_align.hip): ``align_pose`` iterates that step on the device -- up to
``align_steps`` times the sums at the working pose and a one-thread float64 kernel that solves the damped normal
equations, bounds the step, moves the pose (the Cayley map, not ``apply_twist``'s exponential: it needs no sine or
cosine, so the tests' numpy mirror gives the same bits) and writes the float32 copy the next sums are taken at -- and
returns a ``PoseAlignment``: the pose, a status and the history of the steps.  ``Localizer(mode="map")`` aligns the
motion model's start pose with it before the splat tracker runs.  It changes nothing in the map.  One more entry point,
one fixed sequence of launches; one read-back.

Photometric term (``MapConfig.photo_scale``, csrc/map_photo.hip): those normal equations read nothing but depth, and a
wall leaves three moves of the camera open.  With an ``intensity`` image of the frame (``intensity(rgb)``, one kernel)
``pose_information``, ``align_pose``, ``align_poses`` and ``loop_constraint`` add one photometric equation per used row
-- the row's colour against the image at its own pixel, ``photo_scale`` metres per unit of intensity -- into the same 30
integers; the step kernels and everything on the host read them as before.  Three more entry points, the launch
sequences of their twins; without an image the calls are exactly what they were.

Exposure compensation (``MapConfig.photo_exposure``, csrc/map_exposure.hip): that term compares a row's stored colour
with the frame's intensity as if every frame had one exposure.  ``estimate_exposure`` fits gain * Y_frame + offset to
the colours of the rows the frame sees -- fixed-point sums over the rows and a one-thread float64 solve, a fixed
sequence of launches with one read-back -- and ``apply_exposure`` corrects the frame's rgb with it on the device; the
corrected image is what every consumer above receives.  Two more entry points; nothing else changes.

Trajectory correction (``MapConfig.origins``, csrc/map_correct.hip): a row is written into the world once, at the
estimate of the frame that saw it.  With the option every row carries the index of that frame (``origins``), and
``correct`` moves the rows of every frame by that frame's rigid transform -- the one that takes its old pose to its
corrected one -- in place, with the stored keyframe poses.  ``spread_correction`` makes such transforms of one loop
constraint (the correction of the last frame, spread over the frames since the first by path length);
``loop_constraint`` measures one against the old part of the map (``align_pose`` and ``score_poses`` on the rows up
to a frame, a prefix of the map).  When to close a loop stays the caller's decision.  One more entry point; ``correct``
reads back once.

Covisibility and the pose graph (``MapConfig.loop``, csrc/map_covis.hip): ``covisibility`` bins the three verdicts of
``score_poses`` for one pose by the frame every row came from -- which frames' rows a depth frame sees, and whether they
agree with it -- in one launch with one read-back; ``optimise_pose_graph`` makes a trajectory consistent with its
tracked odometry and any number of loop constraints at once, least squares on SE(3) in float64 on the host.
``Localizer(mode="map")`` finds, measures and closes loops with the two (localizer.py)."""
from __future__ import annotations

import functools
import math
from dataclasses import dataclass
from typing import Optional, Tuple

import numpy as np
import torch
from torch import Tensor

from . import _lib

MERGE_CELL_MAX = 2 ** 20 - 1  # |cell| along an axis that the 3 x 21-bit voxel key of csrc/map_merge.hip holds
MERGE_SCENE_M = 100.0  # a merge_voxel that leaves that range within this distance of the origin is refused
SCORE_MAX_POSES = 64  # poses one call of csrc/map_score.hip scores (gsl_map_score_max_poses())
PLACE_CELLS = 192  # the 16 x 12 cells of a descriptor of csrc/map_place.hip (gsl_map_place_cells())
PLACE_GW, PLACE_GH = 16, 12
PLACE_MAX_KEYFRAMES = 256  # keyframes one call of gsl_map_place_match compares (GSL_MAP_PLACE_MAX_KEYFRAMES)
PLACE_SHIFTS = tuple((sx, sy) for sy in (-1, 0, 1) for sx in (-2, -1, 0, 1, 2))  # the kernel's order
INFO_VALUES = 30  # int64 sums one call of csrc/map_info.hip leaves (gsl_map_info_values())
INFO_ONE = float(2 ** 20)  # their fixed point
# The default of MapConfig.info_min_eig.  An eigenvalue of H / used is the mean over the rows used of the squared
# component of J along a direction: for a translation that of the unit normals (1 / 3 each in a corner seen evenly, 0
# along a wall), for a rotation that of p x n in m^2.  1e-3 is normals within 1.8 degrees (rms) of perpendicular to a
# direction -- a wall, to the eye -- and 2000 times the 2^-21 that the rounding of a fixed-point term can add to a mean
INFO_MIN_EIG = 1e-3
INFO_PHOTO_MAX_SCALE = 16.0  # photo_scale one call of csrc/map_photo.hip takes at the most (its overflow bound)
ALIGN_MAX_STEPS = 32  # iterations one call of csrc/map_align.hip runs at the most (gsl_map_align_max_steps())
ALIGN_STATE_WORDS, ALIGN_ROW_WORDS = 14, 10  # 8-byte words of its state and of a history row (include/gsloc_hip.h)
ALIGN_BATCH_MAX_POSES = 16  # poses one call of csrc/map_align_batch.hip aligns (gsl_map_align_batch_max_poses())
ALIGN_MIN_USED = 7  # rows: six unknowns and one to spare, as PoseInformation.weak
ALIGN_STATUS = ("STEPPED", "CONVERGED", "FEW", "SINGULAR", "TOO_FAR")  # GSL_MAP_ALIGN_*
PYRAMID_MAX_LEVELS = 4  # levels above the frame one call of csrc/map_pyramid.hip builds (GSL_MAP_PYRAMID_MAX_LEVELS)
PYRAMID_MIN_SIDE = 4  # pixels: the coarsest level is at least this wide and high
EXPOSURE_VALUES, EXPOSURE_RECORD_WORDS = 7, 6  # int64 sums and 8-byte words per pass of csrc/map_exposure.hip
EXPOSURE_MAX_PASSES = 4  # passes one call of it runs at the most (GSL_MAP_EXPOSURE_MAX_PASSES)
EXPOSURE_STATUS = ("OK", "FEW", "FLAT", "RANGE")  # GSL_MAP_EXPOSURE_*


@dataclass
class PoseInformation:
    """The normal equations of a pose from the map's rows against a depth frame (``GaussianMap.pose_information``), for
    a left perturbation w2c' = exp(xi^) w2c with xi = (omega [rad], upsilon [m]) in the camera's frame: H = sum J J^T
    [6,6] and g = sum J r [6] over the rows used, float64 (the kernel's integers / 2^20); rss = sum r^2 in m^2; the rows
    used and tested; min_eig: the bound ``weak`` takes by default.  With a photometric term (``intensity=``) H, g and
    rss hold geometry plus colour, a colour residual counted as photo_scale metres per unit of intensity; photo_used:
    the rows that gave a photometric equation (all of them among ``used``), photo_rss: their share of rss."""
    H: np.ndarray
    g: np.ndarray
    rss: float
    used: int
    tested: int
    min_eig: float = INFO_MIN_EIG
    photo_used: int = 0
    photo_rss: float = 0.0

    @property
    def eigenvalues(self) -> np.ndarray:
        """Of H / used, ascending (zeros when no row was used)."""
        if self.used == 0:
            return np.zeros(6)
        return np.linalg.eigvalsh(self.H / float(self.used))

    def weak(self, min_eig: Optional[float] = None) -> bool:
        """Fewer than 7 rows used (six unknowns and one degree of freedom for sigma), or the smallest eigenvalue of
        H / used below min_eig: some move of the camera that the frame does not pin down."""
        bound = self.min_eig if min_eig is None else float(min_eig)
        return self.used < 7 or not float(self.eigenvalues[0]) >= bound

    def covariance(self) -> Optional[np.ndarray]:
        """sigma^2 H^-1 [6,6] with sigma^2 = rss / (used - 6), in (rad, m); None when weak.  With a photometric term
        rss is the sum over used + photo_used equations while the divisor stays used - 6: sigma^2 is overstated by up
        to a factor of two (every used row also gave a colour equation), never understated."""
        if self.weak():
            return None
        return (self.rss / float(self.used - 6)) * np.linalg.inv(self.H)

    def step(self) -> Optional[np.ndarray]:
        """The Gauss-Newton step -H^-1 g [6] = (omega, upsilon) (``apply_twist``); None when weak."""
        if self.weak():
            return None
        return -np.linalg.solve(self.H, self.g)


def information_from_sums(sums, min_eig: float = INFO_MIN_EIG, extra=None) -> PoseInformation:
    """The ``PoseInformation`` of the 30 int64 sums of csrc/map_info.hip (the upper triangle of H row-major, g, the
    residual sum, the rows used and tested); extra: None, or the two int64 of gsl_map_pose_info_photo."""
    sums = np.asarray(sums, dtype=np.int64)
    H, k = np.zeros((6, 6)), 0
    for a in range(6):
        for b in range(a, 6):
            H[a, b] = H[b, a] = float(sums[k]) / INFO_ONE
            k += 1
    photo = (0, 0.0) if extra is None else (int(extra[0]), float(extra[1]) / INFO_ONE)
    return PoseInformation(H, sums[21:27].astype(np.float64) / INFO_ONE, float(sums[27]) / INFO_ONE, int(sums[28]),
                           int(sums[29]), min_eig, *photo)


@dataclass
class PoseAlignment:
    """What ``GaussianMap.align_pose`` returns.  c2w: float32 [4,4] on the map's device, the float64 inverse of w2c64
    rounded once; w2c64: float64 [4,4] numpy, the device's world-to-camera pose after the last applied step (the exact
    widening of the float32 start when none was); status: the last iteration's, one of ``ALIGN_STATUS`` -- STEPPED
    (every iteration moved the pose and the last step was still above the stop tolerance), CONVERGED (a step within it
    was applied), FEW (fewer than 7 rows used), SINGULAR (a pivot of the damped normal equations not above 0), TOO_FAR
    (a step beyond the bound; not applied); the last three leave the pose where the step before them put it.  steps:
    the steps applied; used / tested: the rows of the last iteration's sums, at the final pose when the run stopped
    early; history: per iteration (status, used, tested, rss [m^2], xi [6] float64 = (omega [rad], upsilon [m]))."""
    c2w: Tensor
    w2c64: np.ndarray
    status: str
    steps: int
    used: int
    tested: int
    history: list
    # ``align_poses`` only: closed -- the device took the sums once more at the final pose (its ``done`` word reads 2);
    # final: the ``PoseInformation`` of those sums, the normal equations at c2w, present when closed
    closed: bool = False
    final: Optional[PoseInformation] = None
    # coarse to fine (``levels=``): every field above is level 0's; level_history -- per level from the coarsest to
    # level 0, that level's history in the format above (the last entry is ``history``); level_steps -- the steps each of
    # them applied, in the same order.  Both None without levels
    level_history: Optional[list] = None
    level_steps: Optional[list] = None

    @property
    def moved(self) -> bool:
        """The pose is a new one: at least one step was applied and no iteration refused."""
        return self.steps > 0 and self.status in ("STEPPED", "CONVERGED")


def pyramid_sizes(width: int, height: int, levels: int) -> list:
    """[(W_l, H_l)] of levels 0 .. levels: every level halves the one before it, an odd last column or row dropped.
    Refused (ValueError) for what gsl_map_pyramid refuses."""
    if isinstance(levels, bool) or not isinstance(levels, (int, np.integer)) or not 1 <= int(levels) <= PYRAMID_MAX_LEVELS:
        raise ValueError(f"levels {levels!r}: a whole number of pyramid levels, 1 .. {PYRAMID_MAX_LEVELS}")
    levels = int(levels)
    if (width >> levels) < PYRAMID_MIN_SIDE or (height >> levels) < PYRAMID_MIN_SIDE:
        raise ValueError(f"levels {levels}: level {levels} of a {width} x {height} frame is {width >> levels} x "
                         f"{height >> levels}, smaller than {PYRAMID_MIN_SIDE} x {PYRAMID_MIN_SIDE}")
    return [(width >> l, height >> l) for l in range(levels + 1)]


def pyramid_intrinsics(intr, levels: int) -> list:
    """[(fx, fy, cx, cy)] of levels 0 .. levels as float32 values: pixel u lies at the integer u, the centre of a 2 x 2
    block at 2 i + 0.5, so fx' = fx * 0.5f, cx' = (cx - 0.5f) * 0.5f (fy, cy likewise), each operation rounded once."""
    half = np.float32(0.5)
    out = [tuple(np.float32(a) for a in intr)]
    for _ in range(int(levels)):
        fx, fy, cx, cy = out[-1]
        out.append((fx * half, fy * half, (cx - half) * half, (cy - half) * half))
    return [tuple(float(a) for a in level) for level in out]


@dataclass
class FramePyramid:
    """What ``GaussianMap.pyramid`` returns.  depths / intensities: per level 0 .. levels a float32 [H_l, W_l] tensor on
    the map's device -- level 0 the inputs themselves, the others views into one packed buffer per image (intensities
    None for a depth-only pyramid); sizes: (W_l, H_l) per level; keep: 1 - rho_p, the float32 value the kernel was given;
    intrs: per level (fx, fy, cx, cy) as float32 values, when K was given (``pyramid_intrinsics``)."""
    levels: int
    depths: list
    intensities: Optional[list]
    sizes: list
    keep: float
    intrs: Optional[list] = None


@dataclass
class Exposure:
    """The affine brightness model of a frame against the map (``GaussianMap.estimate_exposure``): gain * Y_frame + offset
    ~ Y_row over the rows the frame sees, the float32 pair the device holds and ``apply_exposure`` applies.  status: of
    the last pass -- "OK", "FEW" (fewer rows used than ``exposure_min_used``), "FLAT" (the variance of the frame's
    intensities over them is not above ``exposure_min_var``: a constant image says nothing about gain) or "RANGE" (the
    solution lies outside ``exposure_gain`` / ``exposure_max_offset``).  A pass that is not OK leaves the pair as the
    pass before left it (the identity, if it was the first) and ends the estimate: only an OK estimate is a correction
    to apply.  used, seen: the rows of the last pass; rss: its residual sum of squares, in squared intensity;
    history: per pass (status, used, seen, g, b, rss) with the float64 solution."""
    gain: float
    offset: float
    status: str
    used: int = 0
    seen: int = 0
    rss: float = 0.0
    history: Optional[list] = None

    @property
    def ok(self) -> bool:
        return self.status == "OK"


def apply_twist(c2w, xi) -> Tensor:
    """The camera-to-world pose after the left perturbation w2c' = exp(xi^) w2c, xi = (omega [rad], upsilon [m]) in the
    camera's frame: c2w' = c2w exp(-xi^).  The exponential of se(3) in float64 (Rodrigues; the series where |omega| is
    tiny); returned in c2w's dtype, on its device."""
    c2w = torch.as_tensor(c2w)
    if c2w.shape != (4, 4):
        raise ValueError(f"c2w is {tuple(c2w.shape)}, not (4, 4)")
    xi = -np.asarray(xi, dtype=np.float64).reshape(6)
    w, v = xi[:3], xi[3:]
    th = float(np.linalg.norm(w))
    K = np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])
    if th < 1e-6:
        a, b, c = 1.0 - th * th / 6.0, 0.5 - th * th / 24.0, 1.0 / 6.0 - th * th / 120.0
    else:
        a, b, c = math.sin(th) / th, (1.0 - math.cos(th)) / (th * th), (th - math.sin(th)) / (th ** 3)
    E = np.eye(4)
    E[:3, :3] = np.eye(3) + a * K + b * (K @ K)
    E[:3, 3] = (np.eye(3) + b * K + c * (K @ K)) @ v
    out = c2w.detach().cpu().double().numpy() @ E
    return torch.from_numpy(out).to(dtype=c2w.dtype if c2w.is_floating_point() else torch.float64, device=c2w.device)


@dataclass
class LoopConstraint:
    """What ``GaussianMap.loop_constraint`` returns.  alignment: the ``PoseAlignment`` of the given pose against the
    prefix; rows: the prefix, ``rows_up_to(upto_frame)``; scores / aligned_scores: int64 [3] (tested, agree, front) of
    the given and of the aligned pose against that prefix."""
    alignment: PoseAlignment
    rows: int
    scores: np.ndarray
    aligned_scores: np.ndarray


def _hat(w) -> np.ndarray:
    return np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])


def _se3_log(T: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
    """(omega, upsilon) with exp((omega, upsilon)^) = T, for a rotation below 90 degrees: float64, closed form, the
    series where the angle is tiny."""
    R, t = T[:3, :3], T[:3, 3]
    s = 0.5 * np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])  # sin(th) * axis
    sin, cos = float(np.linalg.norm(s)), 0.5 * (float(np.trace(R)) - 1.0)
    th = math.atan2(sin, cos)
    if th < 1e-4:
        w = s * (1.0 + th * th / 6.0 + 7.0 * th ** 4 / 360.0)
        c = 1.0 / 12.0 + th * th / 720.0 + th ** 4 / 30240.0
    else:
        w = s * (th / sin)
        # of th alone, not of sin and cos: a rotation that is orthonormal to float32 only has a sine and a cosine that
        # disagree in the eighth digit, and 1 - cos would carry that into the fourth
        c = (1.0 - 0.5 * th / math.tan(0.5 * th)) / (th * th)
    Kw = _hat(w)
    return w, (np.eye(3) - 0.5 * Kw + c * (Kw @ Kw)) @ t


def _se3_exp(w: np.ndarray, v: np.ndarray) -> np.ndarray:
    """[4,4] float64: the exponential of the twist (omega, upsilon) (Rodrigues; the series where |omega| is tiny)."""
    th = float(np.linalg.norm(w))
    Kw = _hat(w)
    if th < 1e-4:
        a, b, c = 1.0 - th * th / 6.0, 0.5 - th * th / 24.0, 1.0 / 6.0 - th * th / 120.0
    else:
        a, b, c = math.sin(th) / th, (1.0 - math.cos(th)) / (th * th), (th - math.sin(th)) / (th ** 3)
    E = np.eye(4)
    E[:3, :3] = np.eye(3) + a * Kw + b * (Kw @ Kw)
    E[:3, 3] = (np.eye(3) + b * Kw + c * (Kw @ Kw)) @ v
    return E


def spread_correction(poses, first: int, last: int, delta, by: str = "path") -> np.ndarray:
    """One loop constraint spread over a trajectory.  poses [n,4,4]: the camera-to-world poses so far; delta [4,4]: the
    correction of frame ``last`` in the world, c2w_new(last) = delta c2w_old(last); frame ``first`` and the frames before
    it are right as they are.  Returns D [n,4,4] float64 with c2w_new(k) = D_k c2w_old(k), D_k = exp(s_k log(delta)) on
    SE(3): s_k = 0 for k <= first -- those D_k are the identity matrix itself, so that the rows of these frames keep
    every bit in ``GaussianMap.correct`` -- s_k = 1 for k >= last, and in between the length of the path of the camera
    centres from ``first`` to k over that from ``first`` to ``last`` (by="path"), or (k - first) / (last - first)
    (by="index", and when the path has no length).  The drift of a tracker accumulates with the motion it tracked,
    not with the count of frames: a camera that stood still for a while has not drifted there.  A ValueError for
    first >= last, an index outside the poses, a delta that is not a rigid transform, or one that turns by 90 degrees
    or more (no loop constraint worth closing is that far off, and the logarithm stays well conditioned)."""
    P = torch.as_tensor(poses).detach().cpu().double().numpy()
    if P.ndim != 3 or P.shape[1:] != (4, 4):
        raise ValueError(f"poses are {P.shape}, not (n, 4, 4)")
    n = len(P)
    for name, v in (("first", first), ("last", last)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not 0 <= v < n:
            raise ValueError(f"{name} {v!r}: an index into the {n} poses")
    first, last = int(first), int(last)
    if first >= last:
        raise ValueError(f"first {first} is not before last {last}")
    if by not in ("path", "index"):
        raise ValueError(f"by {by!r}: 'path' or 'index'")
    D = torch.as_tensor(delta).detach().cpu().double().numpy()
    if D.shape != (4, 4) or not np.isfinite(D).all():
        raise ValueError("delta is not a finite [4,4] matrix")
    R = D[:3, :3]
    if (np.abs(R.T @ R - np.eye(3)).max() > 1e-5 or np.linalg.det(R) <= 0.0
            or np.abs(D[3] - np.array([0.0, 0.0, 0.0, 1.0])).max() > 1e-9):
        raise ValueError("delta is not a rigid transform (R^T R = 1 within 1e-5, det R > 0, last row 0 0 0 1)")
    if not np.trace(R) - 1.0 > 1e-9:  # cos(angle) = (trace - 1) / 2; a quarter turn's own rounding does not pass
        raise ValueError("delta turns by 90 degrees or more")
    w, v = _se3_log(D)
    span = np.arange(first, last + 1)
    s = (span - first) / float(last - first)
    if by == "path":
        centres = P[first:last + 1, :3, 3]
        along = np.concatenate([[0.0], np.cumsum(np.linalg.norm(np.diff(centres, axis=0), axis=1))])
        if not np.isfinite(along).all():
            raise ValueError("poses: a camera centre between first and last is not finite")
        if along[-1] > 0.0:
            s = along / along[-1]
    out = np.tile(np.eye(4), (n, 1, 1))
    for k in range(first + 1, n):
        sk = 1.0 if k >= last else float(s[k - first])
        if sk > 0.0:
            out[k] = _se3_exp(sk * w, sk * v)
    return out


@dataclass
class PoseGraphResult:
    """What ``optimise_pose_graph`` returns.  poses: float64 [n,4,4]; cost_before / cost_after: the weighted sum of
    squared residuals sum w r^T r over all edges at the given and at the returned poses; iterations: the linear solves
    whose step was taken; converged: the last step stayed within the tolerance (False: ``iters`` ran out, or no damping
    made the cost fall); loop_residuals: float64 [len(loops)], the norm of every loop edge's residual (rad and m in one
    vector, as the cost has them) at the returned poses."""
    poses: np.ndarray
    cost_before: float
    cost_after: float
    iterations: int
    converged: bool
    loop_residuals: np.ndarray


class _TooFar(ValueError):
    pass


def _bernoulli_over_factorial(upto: int) -> list:
    """B_n / n! for n = 0 .. upto (B_1 = -1/2), exact fractions rounded once."""
    from fractions import Fraction

    B, fact, out = [], Fraction(1), []
    for m in range(upto + 1):
        B.append(Fraction(1) if m == 0 else -sum(Fraction(math.comb(m + 1, k)) * B[k] for k in range(m)) / (m + 1))
        fact = fact * m if m > 0 else fact
        out.append(float(B[m] / fact))
    return out


_B_OVER_FACT = _bernoulli_over_factorial(30)


def _jr_inv(r: np.ndarray) -> np.ndarray:
    """[6,6]: the inverse right Jacobian of SE(3) at the twist r = (omega, upsilon), log(exp(r^) exp(d^)) = r + Jr^-1 d
    to first order: the series sum B_n / n! (-ad_r)^n, which converges for |omega| < 2 pi and is at rounding after 30
    terms for the rotations below 90 degrees that an edge is allowed."""
    ad = np.zeros((6, 6))
    ad[:3, :3] = ad[3:, 3:] = _hat(r[:3])
    ad[3:, :3] = _hat(r[3:])
    out, sq = np.eye(6) + 0.5 * ad, ad @ ad
    term = sq
    for n in range(2, len(_B_OVER_FACT), 2):
        out = out + _B_OVER_FACT[n] * term
        term = term @ sq
    return out


def _adjoint(T: np.ndarray) -> np.ndarray:
    """[6,6]: T exp(x^) T^-1 = exp((Ad x)^) for twists x = (omega, upsilon)."""
    R, out = T[:3, :3], np.zeros((6, 6))
    out[:3, :3] = out[3:, 3:] = R
    out[3:, :3] = _hat(T[:3, 3]) @ R
    return out


def _rigid(M, what: str) -> np.ndarray:
    """M as a float64 [4,4] rigid transform, refused otherwise (the bounds of ``spread_correction``)."""
    M = torch.as_tensor(M).detach().cpu().double().numpy()
    if M.shape != (4, 4) or not np.isfinite(M).all():
        raise ValueError(f"{what} is not a finite [4,4] matrix")
    R = M[:3, :3]
    if (np.abs(R.T @ R - np.eye(3)).max() > 1e-5 or np.linalg.det(R) <= 0.0
            or np.abs(M[3] - np.array([0.0, 0.0, 0.0, 1.0])).max() > 1e-9):
        raise ValueError(f"{what} is not a rigid transform (R^T R = 1 within 1e-5, det R > 0, last row 0 0 0 1)")
    return M


def optimise_pose_graph(poses, odometry, loops, fixed_upto: int, by: str = "index", iters: int = 30,
                        tol: float = 1e-12, solver: Optional[str] = None) -> PoseGraphResult:
    """A trajectory made consistent with several loop constraints at once: least squares over a pose graph on SE(3),
    float64, on the host (the nodes number in the hundreds, once per closure).

    poses [n,4,4]: the camera-to-world poses so far, the start.  odometry [n-1,4,4]: Z_k, the relative pose
    T_k^-1 T_k+1 as it was tracked.  loops: (i, j, Z, weight) with i < j, Z [4,4] the measured T_i^-1 T_j and weight
    above 0.  The residual of an edge (i, j, Z) is r = log(Z^-1 T_i^-1 T_j) = (omega, upsilon), and sum w r^T r is
    minimised by Gauss-Newton with the right perturbation T_k <- T_k exp(d_k^) and the exact Jacobians (the inverse
    right Jacobian of SE(3): the residuals of a drifted trajectory do not vanish at the minimum, and a first-order
    Jacobian would stop beside it); a step under which the cost would rise is taken again with Levenberg's damping,
    lambda diag(H), ten times stronger each time.  Odometry weights: 1 (by="index"); or the mean step length over the
    edge's own -- the length of Z_k's translation, floored at 1 % of the mean -- (by="path", and "index" when the path
    has no length): drift accumulates with the motion that was tracked.  The nodes k <= fixed_upto are not variables
    and come back with every bit.  It stops when a step was taken under which the cost fell by no more than ``tol`` of
    itself, or a step within 1e-11 (rad, m), or after ``iters`` steps.  solver: "sparse" (scipy.sparse, the normal
    equations are block-banded but for the loops), "dense" (numpy), None: sparse where scipy imports.

    A ValueError for poses, Z that are not finite rigid transforms, a wrong count of odometry edges, an index outside the
    poses, i >= j, a weight that is not finite and above 0, and for an edge whose residual at the start turns by 90
    degrees or more (``spread_correction``: no constraint worth closing is that far off)."""
    P = torch.as_tensor(poses).detach().cpu().double().numpy()
    if P.ndim != 3 or P.shape[0] < 1 or P.shape[1:] != (4, 4):
        raise ValueError(f"poses are {P.shape}, not (n >= 1, 4, 4)")
    if not np.isfinite(P).all():
        raise ValueError("poses: some entry is not finite")
    n = len(P)
    if isinstance(fixed_upto, bool) or not isinstance(fixed_upto, (int, np.integer)) or not 0 <= fixed_upto < n:
        raise ValueError(f"fixed_upto {fixed_upto!r}: an index into the {n} poses (some node has to hold the graph)")
    if by not in ("path", "index"):
        raise ValueError(f"by {by!r}: 'path' or 'index'")
    if solver not in (None, "sparse", "dense"):
        raise ValueError(f"solver {solver!r}: 'sparse', 'dense' or None")
    if isinstance(iters, bool) or not isinstance(iters, (int, np.integer)) or iters < 1:
        raise ValueError(f"iters {iters!r}: a whole number of steps, at least 1")
    if not (isinstance(tol, (int, float)) and math.isfinite(tol) and tol >= 0):
        raise ValueError(f"tol {tol!r}: finite and not negative")
    odo = [_rigid(Z, f"odometry[{k}]") for k, Z in enumerate(odometry)]
    if len(odo) != n - 1:
        raise ValueError(f"{len(odo)} odometry edges for {n} poses: one per step, {n - 1}")
    weights = np.ones(n - 1)
    if by == "path" and n > 1:
        steps = np.array([np.linalg.norm(Z[:3, 3]) for Z in odo])
        if steps.mean() > 0.0:
            weights = steps.mean() / np.maximum(steps, 0.01 * steps.mean())
    edges = [(k, k + 1, np.linalg.inv(odo[k]), float(weights[k])) for k in range(n - 1)]
    for e, loop in enumerate(loops):
        if len(loop) != 4:
            raise ValueError(f"loops[{e}]: (i, j, Z, weight)")
        i, j, Z, w = loop
        for name, v in (("i", i), ("j", j)):
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not 0 <= v < n:
                raise ValueError(f"loops[{e}]: {name} {v!r} is no index into the {n} poses")
        if i >= j:
            raise ValueError(f"loops[{e}]: i {i} is not before j {j}")
        if isinstance(w, bool) or not isinstance(w, (int, float, np.floating, np.integer)) \
                or not (math.isfinite(w) and w > 0):
            raise ValueError(f"loops[{e}]: weight {w!r}: finite and above 0")
        edges.append((int(i), int(j), np.linalg.inv(_rigid(Z, f"loops[{e}]: Z")), float(w)))
    first, m = int(fixed_upto) + 1, n - int(fixed_upto) - 1  # the variables: nodes first .. n - 1

    def residuals(T, jacobians: bool):
        """(cost, [r per edge], [(Ji, Jj) per edge])."""
        cost, rs, Js = 0.0, [], []
        for i, j, Zinv, w in edges:
            E = Zinv @ np.linalg.inv(T[i]) @ T[j]
            if not np.trace(E[:3, :3]) - 1.0 > 1e-9:
                raise _TooFar(f"the edge ({i}, {j}) is off by a turn of 90 degrees or more")
            r = np.concatenate(_se3_log(E))
            cost += w * float(r @ r)
            rs.append(r)
            if jacobians:
                Jj = _jr_inv(r)
                Js.append((-Jj @ _adjoint(np.linalg.inv(T[j]) @ T[i]), Jj))
        return cost, rs, Js

    def solve(blocks, g, lam):
        """(H + lam diag H) d = -g, H from its 6 x 6 blocks (a, b, block), duplicates summed."""
        use_sparse = solver == "sparse"
        if solver is None:
            try:
                import scipy.sparse  # noqa: F401
                use_sparse = True
            except ImportError:
                use_sparse = False
        if use_sparse:
            from scipy.sparse import coo_matrix, diags
            from scipy.sparse.linalg import spsolve

            rows = np.concatenate([(6 * a + np.arange(6))[:, None].repeat(6, 1).ravel() for a, _, _ in blocks])
            cols = np.concatenate([(6 * b + np.arange(6))[None, :].repeat(6, 0).ravel() for _, b, _ in blocks])
            H = coo_matrix((np.concatenate([B.ravel() for _, _, B in blocks]), (rows, cols)), shape=(6 * m, 6 * m)).tocsc()
            if lam > 0.0:
                H = H + diags(lam * H.diagonal()).tocsc()
            return np.asarray(spsolve(H, -g)).reshape(-1)
        H = np.zeros((6 * m, 6 * m))
        for a, b, B in blocks:
            H[6 * a:6 * a + 6, 6 * b:6 * b + 6] += B
        if lam > 0.0:
            H[np.diag_indices(6 * m)] *= 1.0 + lam
        return np.linalg.solve(H, -g)

    T = P.copy()
    try:
        cost, rs, Js = residuals(T, True)
    except _TooFar as err:
        raise ValueError(str(err)) from None
    before, done, converged, lam = cost, 0, m == 0, 0.0
    while not converged and done < int(iters):
        blocks, g = [], np.zeros(6 * m)
        for (i, j, _, w), r, (Ji, Jj) in zip(edges, rs, Js):
            var = [(k - first, J) for k, J in ((i, Ji), (j, Jj)) if k >= first]
            for a, Ja in var:
                g[6 * a:6 * a + 6] += w * (Ja.T @ r)
                for b, Jb in var:
                    blocks.append((a, b, w * (Ja.T @ Jb)))
        if not blocks:
            converged = True
            break
        taken = False
        while True:
            d = solve(blocks, g, lam).reshape(m, 6)
            size = float(np.abs(d).max()) if np.isfinite(d).all() else math.inf
            cand = T.copy()
            for a in range(m):
                cand[first + a] = T[first + a] @ _se3_exp(d[a, :3], d[a, 3:])
            try:
                c_cost, c_rs, c_Js = residuals(cand, True) if math.isfinite(size) else (math.inf, None, None)
            except _TooFar:
                c_cost = math.inf
            if c_cost <= cost:
                fell = cost - c_cost
                T, cost, rs, Js, taken = cand, c_cost, c_rs, c_Js, True
                converged = fell <= tol * (cost + fell) or size <= 1e-11
                lam = lam / 10.0 if lam > 1e-12 else 0.0
                break
            if size <= 1e-11:  # the cost cannot fall any further: what is left is its rounding
                converged = True
                break
            lam = max(10.0 * lam, 1e-6)
            if lam > 1e12:
                break
        if not taken:
            break
        done += 1
    loop_r = np.array([float(np.linalg.norm(r)) for r in rs[n - 1:]])
    return PoseGraphResult(T, float(before), float(cost), done, bool(converged), loop_r)


OCCL_CELLS = (1, 2, 4, 8, 16)  # the cell sizes of the occlusion z-buffer, pixels (csrc/map_occl.hip)


@dataclass
class MapConfig:
    alpha_min: float = 0.5  # a pixel the map renders with less alpha is not covered
    depth_rho: float = 0.05  # a pixel observed more than this fraction in front of the map's depth is a new surface
    capacity: Optional[int] = None  # rows; None: 4 * W * H
    # Localizer(mode="map"): track against the rows in view from the start pose, the image widened by this many pixels
    # on every side (None: against every live row)
    view_guard_px: Optional[float] = None
    # ... and afterwards count the rows in view from the ESTIMATE, the image widened by this, that the tracked set left
    # out.  A 3 sigma footprint of these clouds is about 7 px wide: a centre up to about 4 px outside still paints inside
    view_reach_px: float = 4.0
    # with view_guard_px: occlusion culling.  The rows in the band are splatted into a z-buffer of view_occlusion_cell_px
    # pixel cells (1, 2, 4, 8 or 16) that keeps the nearest depth per cell, and a row is left out when EVERY cell within
    # view_occlusion_window cells of its own (0 .. 3) holds a depth nearer than (1 - view_occlusion_rho) times the row's:
    # an empty cell, the silhouette of an occluder and a lone ghost row keep it (csrc/map_occl.hip).  A window of 0 lets a
    # slanted surface cull its own far side within a cell, hence 1 (None: the frustum is the only test)
    view_occlusion_rho: Optional[float] = None
    view_occlusion_cell_px: int = 4
    view_occlusion_window: int = 1
    # Localizer(mode="map"): after a frame's insertion, remove the live rows that project into the frame and lie more
    # than this fraction in front of every observed depth within free_window_px pixels of their pixel (None: a map only
    # grows).  The window is what keeps the edge of a surface that is still there when the pose is a little off
    free_rho: Optional[float] = None
    free_window_px: int = 1
    # a bounded map: when a frame's new rows do not fit, the least recently observed rows go first (in map order among
    # rows last observed by the same frame), exactly as many as are short plus evict_headroom; only rows last observed
    # at least evict_min_age frames ago can go (False: the rows that do not fit are dropped and the map is ``full``)
    evict: bool = False
    evict_min_age: int = 1
    evict_headroom: int = 0
    # a row counts as observed by a frame when a pixel within this many pixels of its own shows its depth, within
    # depth_rho either way (or when it lies in the view_reach_px band around the image)
    observe_window_px: int = 1
    # a map with a resolution: the live rows that fall into the same cube of this side, metres in the world, are fused
    # into one row at the first of them -- the mean of their positions and colours, the latest of their stamps -- by
    # GaussianMap.merge, which Localizer(mode="map") calls after the insertion of every merge_every-th frame
    # (None: every inserted row stays one row)
    merge_voxel: Optional[float] = None
    merge_every: int = 1
    # Localizer(mode="map"): relocalisation.  A frame's estimate is held against the map (GaussianMap.score_poses: of
    # the live rows whose own pixel has a depth, those within depth_rho of it AGREE, those nearer are in FRONT) and is
    # accepted when at least reloc_min_tested rows were tested (None: W * H // 16) and agree >= reloc_min_agree *
    # (agree + front).  A rejected estimate is tracked once more, from the best-scoring pose of a grid around the
    # start poses: reloc_levels steps of reloc_rot_deg degrees about, and of reloc_trans metres along, each of the
    # camera's axes, both ways.  A frame rejected again is lost and leaves the map alone
    reloc: bool = False
    # the midpoint of what was measured at 160x120 (NOTES.md, "Relocalisation"): good poses give a share of 0.973 at the
    # least (508 ghost rows of a panel that has gone, in front of what the frame sees), a start 0.3 m off 0.23
    reloc_min_agree: float = 0.6
    reloc_min_tested: Optional[int] = None
    reloc_rot_deg: float = 2.0
    reloc_trans: float = 0.05
    reloc_levels: int = 2
    # with reloc: the reloc_align_top best-scoring candidates of a grid (0: none, at most 16) are aligned to the map in
    # one call (GaussianMap.align_poses) and scored once more; an alignment that moved and that the map scores no worse
    # than its candidate takes the candidate's place before the winner is chosen
    reloc_align_top: int = 0
    # Localizer(mode="map"), with reloc: place recognition.  The map keeps up to keyframe_max keyframes (a ring: the
    # oldest goes first) -- the pose of an inserted frame and a 16 x 12 integer descriptor of its depth image
    # (GaussianMap.add_keyframe) -- and a frame that the relocalisation above leaves lost is compared with all of them
    # (GaussianMap.match_place); the poses of the place_top most similar ones, each turned by the image shift under
    # which it matched best, are the bases of one more candidate grid, scored and tracked from as above
    keyframes: bool = False
    keyframe_max: int = 256
    # a frame becomes a keyframe when its pose is further than keyframe_rot_deg degrees OR further than keyframe_trans
    # metres from every stored keyframe's.  The defaults are half the jump between two frames that the tracker was
    # measured to absorb (12.8 degrees and 32 cm; NOTES.md, "Relocalisation"): a camera within half a spacing of some
    # keyframe is then inside that basin.  The figure comes from one synthetic room
    keyframe_rot_deg: float = 6.0
    keyframe_trans: float = 0.15
    place_top: int = 2  # this many best-matching keyframes become bases: place_top * (1 + 12 reloc_levels) <= 64
    place_min_common: int = 48  # a shift under which fewer cells are valid in both descriptors, a quarter of the 192, does not count
    # Localizer(mode="map"): refinement.  Every row carries the number of depths it is the mean of (GaussianMap.weights),
    # and between a frame's insertion render and its insertion the live rows whose four surrounding pixels all show
    # their depth within refine_rho (None: depth_rho) move along their ray to the running mean of those depths
    # (GaussianMap.refine); a weight stops at refine_max_weight, from where on the mean is an exponential one with
    # gain 1 / (refine_max_weight + 1)
    refine: bool = False
    refine_rho: Optional[float] = None
    refine_max_weight: int = 64
    # Localizer(mode="map"): pose information.  After the relocalisation flow and before anything touches the map, the
    # normal equations of the frame's final estimate are summed over the live rows that agree with their own pixel
    # within info_rho (None: depth_rho) and whose pixel and its four neighbours lie on one plane
    # (GaussianMap.pose_information); the frame reports the covariance of its pose.  Read-only: nothing is gated on it
    info: bool = False
    info_rho: Optional[float] = None
    # the planarity test: the inverse depths of a pixel's two neighbours along a line or a column may miss twice its
    # own by this fraction of it.  A property of the sensor's depth quantisation, not of the scene: on a plane the sum
    # is exact, so the bound has to pass what the sensor's rounding of the three depths adds and nothing more: depths
    # quantised in steps of q metres at the depth d move the sum by up to 2 q / d^2, so info_kappa >= 2 q / d.  1e-3
    # passes float32 depths and a sensor that resolves 1 mm at 2 m, and refuses the creases of a room (NOTES.md, "Pose
    # information"); a sensor with 1 cm steps at 2 m needs 1e-2
    info_kappa: float = 1e-3
    # a frame is weak when fewer than 7 rows were used or the smallest eigenvalue of H / used is below this (None:
    # INFO_MIN_EIG)
    info_min_eig: Optional[float] = None
    # Localizer(mode="map"): pose alignment.  Before the pair is built, the motion model's start pose is aligned to the
    # map by up to align_steps Gauss-Newton steps on those normal equations (GaussianMap.align_pose), and the aligned
    # pose is what the frame starts from when the map scores it no worse than the start (localizer.py).  8 steps: the
    # float64 prototype of a start 5 cm / 3 degrees off was converged at step 7 (NOTES.md, "Pose alignment")
    align: bool = False
    align_steps: int = 8
    # added, times the rows used, to the diagonal of H: the quantity INFO_MIN_EIG bounds -- an eigenvalue of H / used
    # below it belongs to a direction the frame does not pin down, and the damping keeps the step out of it
    align_damping: float = INFO_MIN_EIG
    align_rho: Optional[float] = None  # as info_rho (None: depth_rho); the planarity bound is info_kappa
    # a single step beyond these is not trusted and not taken: the jump between two frames that the tracker was measured
    # to absorb (NOTES.md, "Relocalisation")
    align_max_rot_deg: float = 12.8
    align_max_trans: float = 0.32
    # a step within both has converged: a tenth of the smallest per-frame error of the 160x120 sequence (NOTES.md)
    align_eps_rot_deg: float = 1.5e-4
    align_eps_trans: float = 3e-5
    # with align: a converged alignment may be the frame's pose.  The start goes through GaussianMap.align_poses, and
    # when the alignment is CONVERGED and closed, the map scores it no worse than the start, its final sums used at
    # least align_accept_min_used rows (None: W * H // 16, the default of reloc_min_tested) and are not weak at
    # align_accept_min_eig (None: INFO_MIN_EIG), the aligned pose is the estimate and the tracker does not run
    # (localizer.py; NOTES.md, "Batched alignment")
    align_accept: bool = False
    align_accept_min_used: Optional[int] = None
    align_accept_min_eig: Optional[float] = None
    # trajectory correction: every row carries the index of the frame that appended it (GaussianMap.origins), so that
    # the rows can follow a corrected trajectory (GaussianMap.correct, Localizer.correct_trajectory / close_loop)
    origins: bool = False
    # Localizer(mode="map"), with origins: loops closed in track().  Every loop_every-th frame that is not lost, before
    # anything touches the map, the frame's covisibility with the frames at least loop_min_gap behind it is taken
    # (GaussianMap.covisibility); when those frames' rows are tested loop_min_rows times or more (None: W * H // 8) the
    # estimate is aligned against them alone (GaussianMap.loop_constraint), and the aligned pose becomes a loop edge of
    # the pose graph (Localizer.add_loop, optimise_pose_graph) when it converged, agrees with at least loop_min_agree
    # of the old rows it tests and with no smaller a share than the estimate, and lies at least loop_min_trans metres
    # or loop_min_rot_deg degrees from the estimate.  loop_weight: the weight of a loop edge, an odometry edge has 1 --
    # a constraint measured against the map itself is worth many tracked steps; loop_by: the odometry weights, by
    # "index" or by "path" length (optimise_pose_graph)
    loop: bool = False
    loop_min_gap: int = 30
    loop_every: int = 10
    loop_min_rows: Optional[int] = None
    loop_min_agree: float = 0.9
    loop_min_trans: float = 0.005
    loop_min_rot_deg: float = 0.1
    loop_weight: float = 1e4
    loop_by: str = "index"
    # Localizer(mode="map"): a photometric term in those normal equations (csrc/map_photo.hip).  With photo_scale set,
    # every row that gives a point-to-plane equation also gives one from its colour against the frame's intensity
    # image, in metres: photo_scale metres of depth residual per unit of intensity residual (intensities are 0 .. 1).
    # It goes into the calls that info, align (align_accept, reloc_align_top) and loop already make, so one of the
    # three has to be on.  A textured plane then pins the pose down where depth alone leaves three moves open.  On the
    # textured wall of NOTES.md, "Photometric term", 0.2 -- the documented value to start from -- lifts the three open
    # eigenvalues of H / used to 8e-3 .. 2e-2, eight times INFO_MIN_EIG, and converges in four steps; 0.1 needs seven;
    # 0.05 stays below INFO_MIN_EIG.  None: off, every launch, buffer and number is what it is without the field
    photo_scale: Optional[float] = None
    # a row whose intensity misses the image's by more than this gives no photometric equation: an occluder, a
    # highlight or a wrong row, not a pose error
    photo_max_residual: float = 0.1
    # Localizer(mode="map"): coarse-to-fine alignment on an image pyramid of the frame (csrc/map_pyramid.hip).  With
    # align_levels in 1 .. 4 a frame builds the pyramid of its depth (and of its intensity image, with photo_scale) once,
    # and every alignment of the frame -- of the start pose, of the relocalisation's candidates, of a loop constraint --
    # runs at level align_levels first and then down to the frame itself, align_level_steps steps at the coarse levels
    # (None: align_steps).  Every level halves the frame, and doubles the distance from which the photometric term
    # pulls the right way: on the fine-textured wall of NOTES.md, "Image pyramid", three levels converge from 8 pixels
    # off where one level stops converging between 2 and 4.  It goes into the calls that align (align_accept,
    # reloc_align_top) and loop make, so one of the two has to be on.  pyramid_rho: a 2 x 2 block whose depths differ by
    # more than this fraction of the largest gives no coarse pixel (None: the alignment's rho).  0: off, every launch,
    # buffer and number is what it is without the field
    align_levels: int = 0
    align_level_steps: Optional[int] = None
    pyramid_rho: Optional[float] = None
    # Localizer(mode="map"), with photo_scale: exposure compensation (csrc/map_exposure.hip).  The photometric term
    # holds a row's colour against the frame's intensity as if every frame had the exposure of the first.  With the
    # option a frame's gain and offset, gain * Y_frame + offset ~ Y_row, are estimated against the rows it sees
    # (GaussianMap.estimate_exposure) at its start pose, its rgb is corrected (apply_exposure) and the intensity image,
    # the pyramid and every alignment, pose information and loop constraint of the frame are made from the corrected
    # image; before anything of the frame enters the map the raw image is corrected once more, with the estimate at the
    # frame's final pose, for refine and insert_frame: the map stays in the exposure of its first frame.
    # exposure_passes: 1 .. 4 least-squares passes; from the second on a row whose corrected intensity misses its
    # colour by more than exposure_max_residual is left out.  exposure_rho: a row is seen when its depth is within this
    # fraction of its pixel's (None: align_rho, or 0.05 when that is None).  exposure_saturation: intensities outside
    # this range, of the frame or of the row, are clipped and follow no affine model.  Fewer than exposure_min_used rows,
    # a variance of the frame's intensities not above exposure_min_var, or a solution outside exposure_gain /
    # exposure_max_offset is no estimate: the frame stays as it is and says so.  False: every launch, buffer and number
    # is what it is without the field
    photo_exposure: bool = False
    exposure_passes: int = 2
    exposure_rho: Optional[float] = None
    exposure_max_residual: float = 0.1
    exposure_saturation: Tuple[float, float] = (0.02, 0.98)
    exposure_min_used: int = 256
    exposure_gain: Tuple[float, float] = (0.5, 2.0)
    exposure_max_offset: float = 0.25
    exposure_min_var: float = 1e-4

    def __post_init__(self):
        whole = lambda v: isinstance(v, int) and not isinstance(v, bool)  # noqa: E731
        number = lambda v: not isinstance(v, bool) and isinstance(v, (int, float, np.floating, np.integer))  # noqa: E731
        if not isinstance(self.photo_exposure, bool):
            raise ValueError(f"photo_exposure {self.photo_exposure!r}: True or False")
        if self.photo_exposure and self.photo_scale is None:
            raise ValueError("photo_exposure=True needs photo_scale: the exposure is compensated for the photometric term")
        if not whole(self.exposure_passes) or not 1 <= self.exposure_passes <= EXPOSURE_MAX_PASSES:
            raise ValueError(f"exposure_passes {self.exposure_passes!r}: a whole number of passes, 1 .. "
                             f"{EXPOSURE_MAX_PASSES}")
        if self.exposure_rho is not None and (not number(self.exposure_rho) or not 0.0 <= self.exposure_rho < 1.0):
            raise ValueError(f"exposure_rho {self.exposure_rho!r}: a fraction of the observed depth, inside [0, 1) (or "
                             "None: align_rho, or 0.05)")
        if not number(self.exposure_max_residual) or not 0.0 <= self.exposure_max_residual <= 1.0:
            raise ValueError(f"exposure_max_residual {self.exposure_max_residual!r}: an intensity difference, inside "
                             "[0, 1]")
        _exposure_pair(self.exposure_saturation, "exposure_saturation")
        _exposure_pair(self.exposure_gain, "exposure_gain")
        if not whole(self.exposure_min_used) or self.exposure_min_used < 1:
            raise ValueError(f"exposure_min_used {self.exposure_min_used!r}: a whole number of rows, at least 1")
        for name in ("exposure_max_offset", "exposure_min_var"):
            v = getattr(self, name)
            if not number(v) or not (np.isfinite(v) and v >= 0):
                raise ValueError(f"{name} {v!r}: finite and not negative")
        if not whole(self.align_levels) or not 0 <= self.align_levels <= PYRAMID_MAX_LEVELS:
            raise ValueError(f"align_levels {self.align_levels!r}: a whole number of pyramid levels, 0 .. "
                             f"{PYRAMID_MAX_LEVELS}")
        if self.align_level_steps is not None and (not whole(self.align_level_steps)
                                                   or not 1 <= self.align_level_steps <= ALIGN_MAX_STEPS):
            raise ValueError(f"align_level_steps {self.align_level_steps!r}: a whole number of iterations, 1 .. "
                             f"{ALIGN_MAX_STEPS} (or None: align_steps)")
        if self.pyramid_rho is not None and (not number(self.pyramid_rho) or not 0.0 <= self.pyramid_rho < 1.0):
            raise ValueError(f"pyramid_rho {self.pyramid_rho!r}: a fraction of the largest depth of a block, inside "
                             "[0, 1) (or None: the alignment's rho)")
        if self.align_levels > 0 and not (self.align is True or self.loop is True):
            raise ValueError("align_levels needs align=True or loop=True: the pyramid goes into the alignments that "
                             "those options make")
        if self.photo_scale is not None and (not number(self.photo_scale)
                                             or not 0.0 <= self.photo_scale <= INFO_PHOTO_MAX_SCALE):
            raise ValueError(f"photo_scale {self.photo_scale!r}: metres per unit of intensity, inside [0, "
                             f"{INFO_PHOTO_MAX_SCALE:g}] (or None: no photometric term)")
        if not number(self.photo_max_residual) or not 0.0 <= self.photo_max_residual <= 1.0:
            raise ValueError(f"photo_max_residual {self.photo_max_residual!r}: an intensity difference, inside [0, 1]")
        if self.photo_scale is not None and not (self.info is True or self.align is True or self.loop is True):
            raise ValueError("photo_scale needs info=True, align=True or loop=True: the photometric term goes into the "
                             "normal equations that those options sum")
        if not isinstance(self.origins, bool):
            raise ValueError(f"origins {self.origins!r}: True or False")
        if not isinstance(self.loop, bool):
            raise ValueError(f"loop {self.loop!r}: True or False")
        if self.loop and not self.origins:
            raise ValueError("loop=True needs origins=True: a closed loop moves every row with the frame it came from")
        for name in ("loop_min_gap", "loop_every"):
            if not whole(getattr(self, name)) or getattr(self, name) < 1:
                raise ValueError(f"{name} {getattr(self, name)!r}: a whole number of frames, at least 1")
        if self.loop_min_rows is not None and (not whole(self.loop_min_rows) or self.loop_min_rows < 1):
            raise ValueError(f"loop_min_rows {self.loop_min_rows!r}: a whole number of rows, at least 1 (or None)")
        if not number(self.loop_min_agree) or not 0.0 < self.loop_min_agree <= 1.0:
            raise ValueError(f"loop_min_agree {self.loop_min_agree!r}: a share of the rows tested, inside (0, 1]")
        for name, unit in (("loop_min_trans", "metres"), ("loop_min_rot_deg", "degrees")):
            v = getattr(self, name)
            if not number(v) or not (np.isfinite(v) and v >= 0):
                raise ValueError(f"{name} {v!r}: {unit}, finite and not negative")
        if not number(self.loop_weight) or not (np.isfinite(self.loop_weight) and self.loop_weight > 0):
            raise ValueError(f"loop_weight {self.loop_weight!r}: finite and above 0")
        if self.loop_by not in ("index", "path"):
            raise ValueError(f"loop_by {self.loop_by!r}: 'index' or 'path'")
        if not isinstance(self.align, bool):
            raise ValueError(f"align {self.align!r}: True or False")
        if not whole(self.align_steps) or not 1 <= self.align_steps <= ALIGN_MAX_STEPS:
            raise ValueError(f"align_steps {self.align_steps!r}: a whole number of iterations, 1 .. {ALIGN_MAX_STEPS}")
        if not number(self.align_damping) or not (np.isfinite(self.align_damping) and self.align_damping >= 0):
            raise ValueError(f"align_damping {self.align_damping!r}: an eigenvalue of H / used, finite and not negative")
        if self.align_rho is not None and (not number(self.align_rho) or not 0.0 <= self.align_rho < 1.0):
            raise ValueError(f"align_rho {self.align_rho!r}: a fraction of the observed depth, inside [0, 1) (or None: "
                             "depth_rho)")
        if self.align and self.align_rho is None and not 0.0 <= self.depth_rho < 1.0:
            raise ValueError(f"depth_rho {self.depth_rho}: align holds a row against the observed depth within this "
                             "fraction, inside [0, 1) (or set align_rho)")
        for name, unit in (("align_max_rot_deg", "degrees"), ("align_max_trans", "metres")):
            v = getattr(self, name)
            if not number(v) or not (np.isfinite(v) and v > 0):
                raise ValueError(f"{name} {v!r}: {unit}, finite and above 0")
        for name, unit in (("align_eps_rot_deg", "degrees"), ("align_eps_trans", "metres")):
            v = getattr(self, name)
            if not number(v) or not (np.isfinite(v) and v >= 0):
                raise ValueError(f"{name} {v!r}: {unit}, finite and not negative")
        if not isinstance(self.align_accept, bool):
            raise ValueError(f"align_accept {self.align_accept!r}: True or False")
        if self.align_accept and not self.align:
            raise ValueError("align_accept=True needs align=True: the pose that is accepted is the aligned start")
        if self.align_accept_min_used is not None and (not whole(self.align_accept_min_used)
                                                       or self.align_accept_min_used < ALIGN_MIN_USED):
            raise ValueError(f"align_accept_min_used {self.align_accept_min_used!r}: a whole number of rows, at least "
                             f"{ALIGN_MIN_USED} (or None)")
        if self.align_accept_min_eig is not None and (
                not number(self.align_accept_min_eig)
                or not (np.isfinite(self.align_accept_min_eig) and self.align_accept_min_eig > 0)):
            raise ValueError(f"align_accept_min_eig {self.align_accept_min_eig!r}: an eigenvalue of H / used, finite and "
                             "above 0 (or None)")
        if not isinstance(self.info, bool):
            raise ValueError(f"info {self.info!r}: True or False")
        if self.info_rho is not None and (not number(self.info_rho) or not 0.0 <= self.info_rho < 1.0):
            raise ValueError(f"info_rho {self.info_rho!r}: a fraction of the observed depth, inside [0, 1) (or None: "
                             "depth_rho)")
        if self.info and self.info_rho is None and not 0.0 <= self.depth_rho < 1.0:
            raise ValueError(f"depth_rho {self.depth_rho}: info holds a row against the observed depth within this "
                             "fraction, inside [0, 1) (or set info_rho)")
        if not number(self.info_kappa) or not (np.isfinite(self.info_kappa) and self.info_kappa >= 0):
            raise ValueError(f"info_kappa {self.info_kappa!r}: a fraction of the inverse depth, finite and not negative")
        if self.info_min_eig is not None and (not number(self.info_min_eig) or
                                              not (np.isfinite(self.info_min_eig) and self.info_min_eig > 0)):
            raise ValueError(f"info_min_eig {self.info_min_eig!r}: an eigenvalue of H / used, finite and above 0 (or "
                             "None)")
        if not isinstance(self.refine, bool):
            raise ValueError(f"refine {self.refine!r}: True or False")
        if self.refine_rho is not None and (not number(self.refine_rho) or not 0.0 <= self.refine_rho < 1.0):
            raise ValueError(f"refine_rho {self.refine_rho!r}: a fraction of the observed depth, inside [0, 1) (or None: "
                             "depth_rho)")
        if self.refine and self.refine_rho is None and not 0.0 <= self.depth_rho < 1.0:
            raise ValueError(f"depth_rho {self.depth_rho}: refine holds a row against the observed depth within this "
                             "fraction, inside [0, 1) (or set refine_rho)")
        if not whole(self.refine_max_weight) or not 1 <= self.refine_max_weight <= 2 ** 30:
            raise ValueError(f"refine_max_weight {self.refine_max_weight!r}: a whole number of depths, 1 .. 2^30")
        if not isinstance(self.reloc, bool):
            raise ValueError(f"reloc {self.reloc!r}: True or False")
        if not isinstance(self.keyframes, bool):
            raise ValueError(f"keyframes {self.keyframes!r}: True or False")
        if not whole(self.keyframe_max) or not 1 <= self.keyframe_max <= PLACE_MAX_KEYFRAMES:
            raise ValueError(f"keyframe_max {self.keyframe_max!r}: a whole number of keyframes, 1 .. {PLACE_MAX_KEYFRAMES}")
        if not number(self.keyframe_rot_deg) or not (np.isfinite(self.keyframe_rot_deg) and self.keyframe_rot_deg > 0):
            raise ValueError(f"keyframe_rot_deg {self.keyframe_rot_deg!r}: degrees, finite and above 0")
        if not number(self.keyframe_trans) or not (np.isfinite(self.keyframe_trans) and self.keyframe_trans > 0):
            raise ValueError(f"keyframe_trans {self.keyframe_trans!r}: metres, finite and above 0")
        if not whole(self.place_top) or self.place_top < 1:
            raise ValueError(f"place_top {self.place_top!r}: a whole number of keyframes, at least 1")
        if not whole(self.place_min_common) or not 1 <= self.place_min_common <= PLACE_CELLS:
            raise ValueError(f"place_min_common {self.place_min_common!r}: a whole number of cells, 1 .. {PLACE_CELLS}")
        if self.keyframes and not self.reloc:
            raise ValueError("keyframes=True needs reloc=True: place recognition is what a frame that the "
                             "relocalisation leaves lost is tried with")
        if not number(self.reloc_min_agree) or not 0.0 < self.reloc_min_agree <= 1.0:
            raise ValueError(f"reloc_min_agree {self.reloc_min_agree!r}: a share of the rows judged, inside (0, 1]")
        if self.reloc_min_tested is not None and (not whole(self.reloc_min_tested) or self.reloc_min_tested < 1):
            raise ValueError(f"reloc_min_tested {self.reloc_min_tested!r}: a whole number of rows, at least 1 (or None)")
        if not number(self.reloc_rot_deg) or not (np.isfinite(self.reloc_rot_deg) and self.reloc_rot_deg > 0):
            raise ValueError(f"reloc_rot_deg {self.reloc_rot_deg!r}: degrees, finite and above 0")
        if not number(self.reloc_trans) or not (np.isfinite(self.reloc_trans) and self.reloc_trans > 0):
            raise ValueError(f"reloc_trans {self.reloc_trans!r}: metres, finite and above 0")
        if not whole(self.reloc_levels) or not 1 <= self.reloc_levels <= 2:
            raise ValueError(f"reloc_levels {self.reloc_levels!r}: a whole number of steps per direction, 1 .. 2")
        if not whole(self.reloc_align_top) or not 0 <= self.reloc_align_top <= ALIGN_BATCH_MAX_POSES:
            raise ValueError(f"reloc_align_top {self.reloc_align_top!r}: a whole number of candidates, 0 .. "
                             f"{ALIGN_BATCH_MAX_POSES}")
        if self.reloc_align_top and not self.reloc:
            raise ValueError("reloc_align_top needs reloc=True: the candidates that are aligned are the relocalisation's")
        if self.place_top * (1 + 12 * self.reloc_levels) > SCORE_MAX_POSES:
            raise ValueError(f"place_top {self.place_top!r}: with reloc_levels {self.reloc_levels} that many bases make "
                             f"{self.place_top * (1 + 12 * self.reloc_levels)} candidate poses, one scoring call takes "
                             f"{SCORE_MAX_POSES}")
        if self.reloc and not 0.0 <= self.depth_rho < 1.0:
            raise ValueError(f"depth_rho {self.depth_rho}: reloc holds a row against the observed depth within this "
                             "fraction, inside [0, 1)")
        if self.merge_voxel is not None:
            v = self.merge_voxel
            if not number(v):
                raise ValueError(f"merge_voxel {v!r}: a length in metres (or None)")
            h = np.float32(v)  # the kernel's h and 1 / h are float32
            if not (np.isfinite(h) and h > 0):
                raise ValueError(f"merge_voxel {v!r}: finite and above 0 as a float32")
            with np.errstate(all="ignore"):
                inv_h = np.float32(1.0) / h
            if not np.isfinite(inv_h) or float(np.float32(MERGE_SCENE_M) * inv_h) > MERGE_CELL_MAX:
                raise ValueError(f"merge_voxel {v!r}: a scene of {MERGE_SCENE_M:g} m has more than {MERGE_CELL_MAX} "
                                 f"voxels of that side along an axis, the voxel key holds 21 bits per axis (at least "
                                 f"{MERGE_SCENE_M / MERGE_CELL_MAX:.2e} m)")
        if not whole(self.merge_every) or self.merge_every < 1:
            raise ValueError(f"merge_every {self.merge_every!r}: a whole number of frames, at least 1")
        if not isinstance(self.evict, bool):
            raise ValueError(f"evict {self.evict!r}: True or False")
        if not whole(self.evict_min_age) or not 1 <= self.evict_min_age <= 1023:
            raise ValueError(f"evict_min_age {self.evict_min_age}: a whole number of frames, 1 .. 1023 (the rows of the "
                             "current frame never go; ages are clamped at 1023)")
        if not whole(self.evict_headroom) or self.evict_headroom < 0:
            raise ValueError(f"evict_headroom {self.evict_headroom}: a whole number of rows, not negative")
        if not whole(self.observe_window_px) or not 0 <= self.observe_window_px <= 3:
            raise ValueError(f"observe_window_px {self.observe_window_px}: a whole number of pixels, 0 .. 3")
        if self.evict and not 0.0 <= self.depth_rho < 1.0:
            raise ValueError(f"depth_rho {self.depth_rho}: evict holds a row against the observed depth within this "
                             "fraction, inside [0, 1)")
        if self.free_rho is not None and not 0.0 < self.free_rho < 1.0:
            raise ValueError(f"free_rho {self.free_rho}: a fraction of the observed depth, inside (0, 1)")
        if not whole(self.free_window_px) or not 0 <= self.free_window_px <= 3:
            raise ValueError(f"free_window_px {self.free_window_px}: a whole number of pixels, 0 .. 3")
        if not self.view_reach_px >= 0.0:
            raise ValueError(f"view_reach_px {self.view_reach_px}: not negative")
        if self.view_guard_px is not None and not self.view_guard_px >= self.view_reach_px:
            raise ValueError(f"view_guard_px {self.view_guard_px} is below view_reach_px {self.view_reach_px}: the band "
                             "that is tracked must hold the band that is checked")
        if self.view_occlusion_rho is not None:
            if not number(self.view_occlusion_rho) or not 0.0 < self.view_occlusion_rho < 1.0:
                raise ValueError(f"view_occlusion_rho {self.view_occlusion_rho!r}: a fraction of a row's depth, inside "
                                 "(0, 1)")
            if self.view_guard_px is None:
                raise ValueError("view_occlusion_rho culls the rows of the guarded view: it needs view_guard_px")
        if not whole(self.view_occlusion_cell_px) or self.view_occlusion_cell_px not in OCCL_CELLS:
            raise ValueError(f"view_occlusion_cell_px {self.view_occlusion_cell_px!r}: one of {OCCL_CELLS} pixels")
        if not whole(self.view_occlusion_window) or not 0 <= self.view_occlusion_window <= 3:
            raise ValueError(f"view_occlusion_window {self.view_occlusion_window!r}: a whole number of cells, 0 .. 3")


def _exposure_pair(v, name: str) -> Tuple[float, float]:
    """``exposure_saturation`` (0 <= lo < hi <= 1) or ``exposure_gain`` (0 < lo <= 1 <= hi < inf) as two floats, refused
    otherwise."""
    number = lambda a: not isinstance(a, bool) and isinstance(a, (int, float, np.floating, np.integer))  # noqa: E731
    ok = isinstance(v, (tuple, list)) and len(v) == 2 and number(v[0]) and number(v[1])
    if ok and name == "exposure_saturation":
        ok = 0.0 <= v[0] < v[1] <= 1.0
    elif ok:
        ok = 0.0 < v[0] <= 1.0 <= v[1] < math.inf
    if not ok:
        what = "0 <= lo < hi <= 1, intensities" if name == "exposure_saturation" else "0 < lo <= 1 <= hi < inf, gains"
        raise ValueError(f"{name} {v!r}: a pair (lo, hi), {what}")
    return float(v[0]), float(v[1])


def _intr_and_pose(K, c2w) -> Tuple[Tuple[float, float, float, float], Tensor]:
    """K [3,3] -> (fx, fy, cx, cy); c2w -> a tensor (dtype and device as given), refused unless it is [4,4]."""
    Kc = torch.as_tensor(K, dtype=torch.float32).cpu()
    c2w = torch.as_tensor(c2w)
    if c2w.shape != (4, 4):
        raise ValueError(f"c2w is {tuple(c2w.shape)}, not (4, 4)")
    return (float(Kc[0, 0]), float(Kc[1, 1]), float(Kc[0, 2]), float(Kc[1, 2])), c2w


def _world_to_camera(c2w: Tensor) -> Tensor:
    """c2w [..., 4, 4] -> float32 on the host: the float64 inverse, rounded to float32 here, once -- the kernels multiply
    and add, nothing else."""
    return torch.from_numpy(np.linalg.inv(c2w.detach().cpu().double().numpy()).astype(np.float32))


class GaussianMap:
    """``insert_frame`` per frame; ``points`` / ``point_colors`` are views of the live prefix (no copy).  A removal
    (``remove_seen_through``) that removes something swaps the buffers behind them: views taken before it are stale."""

    def __init__(self, width: int, height: int, config: MapConfig = MapConfig(), device="cuda"):
        self.W, self.H = int(width), int(height)
        self.cfg = config
        self.device = torch.device(device)
        self.capacity = int(config.capacity) if config.capacity is not None else 4 * self.W * self.H
        if self.capacity <= 0:
            raise ValueError(f"map capacity {self.capacity}: at least one row")
        self.means = torch.zeros(self.capacity, 3, device=self.device)
        self.colors = torch.zeros(self.capacity, 3, device=self.device)
        self.n_live = 0
        self.full = False  # some frame's rows were dropped at the capacity
        # the index of the last frame that observed each row (observe / insert_frame), and of the current frame
        self.stamps = torch.zeros(self.capacity, dtype=torch.int32, device=self.device)
        self.frame_index = 0
        self.last_evicted = 0  # rows the last insert_frame evicted to make room
        # float32 values of the rule, computed here once: the kernel multiplies and compares, nothing else
        self.alpha_min = float(np.float32(config.alpha_min))
        self.keep = float(np.float32(1.0) - np.float32(config.depth_rho))
        self._counters = torch.zeros(2, dtype=torch.int32, device=self.device)
        self._ws = self._alloc_ws()
        # select_view: capacity-sized working buffers and two workspaces, allocated on first use
        self._view = None
        self._view_rows = -1  # n_live at the last select_view: what its ballots describe
        # select_view(occlusion_rho=): two workspaces, four counters and a z-buffer per grid size, allocated on first
        # use; the rho of the last select_view (None: the frustum alone), which view_violations applies as well, and
        # the rows in the band that it left out as occluded
        self._occl = None
        self._view_rho = None
        self.last_view_culled = 0
        # remove_seen_through: the spare pair of buffers, the ids and a workspace, allocated on first use
        self._free = None
        self._free_keep = None if config.free_rho is None else float(np.float32(1.0) - np.float32(config.free_rho))
        self._n_survivors = 0
        # evict: its workspace (not the selection's: the append still needs that one), allocated on first use
        self._evict_ws = None
        # merge: h and 1 / h as the float32 values the kernel is given, its workspace and four counters on first use
        self._merge_h = self._merge_inv_h = None
        if config.merge_voxel is not None:
            h = np.float32(config.merge_voxel)
            self._merge_h, self._merge_inv_h = float(h), float(np.float32(1.0) / h)
        self._merge = None
        # score_poses: 1 + depth_rho as the float32 value the kernel is given; its two buffers on first use
        self.beyond = float(np.float32(1.0) + np.float32(config.depth_rho))
        self._score = None
        # keyframes: the host poses of the ring and how many frames were ever kept; the device table, the query's
        # descriptor and the match's output on first use
        self._kf_poses = np.zeros((int(config.keyframe_max), 4, 4), dtype=np.float32)
        self._kf_made = 0
        self._place = None
        # refine: the number of depths each row is the mean of, 1 - refine_rho as the float32 value the kernel is
        # given and the one counter; nothing of it without the option
        self.weights = self._refine_keep = self._refine_counter = None
        if config.refine:
            rho = config.depth_rho if config.refine_rho is None else config.refine_rho
            self._refine_keep = float(np.float32(1.0) - np.float32(rho))
            self.weights = torch.zeros(self.capacity, dtype=torch.int32, device=self.device)
            self._refine_counter = torch.zeros(1, dtype=torch.int32, device=self.device)
        # pose_information: its 30 sums, on first use
        self._info = None
        self._info_photo = None  # pose_information with intensity=: the 30 sums and the two extra words, on first use
        # align_pose: one buffer of 8-byte words -- state, history, working pose, sums -- and the start pose, on first use
        self._align = None
        self._align_batch = None  # align_poses: the same for 16 poses, on first use
        # align_pose / align_poses with levels=: that buffer and the start pose once per level, by level count, on first use
        self._align_levels: dict = {}
        self._align_batch_levels: dict = {}
        # origins: the index of the frame that appended each row; nothing of it without the option.  The insertions
        # since clear() and the last one's origin; the frame index of the keyframe in every slot (-1: not recorded);
        # correct's two 64-bit counters on first use
        self.origins = None
        if config.origins:
            self.origins = torch.zeros(self.capacity, dtype=torch.int32, device=self.device)
        self._n_inserts, self._last_origin = 0, -1
        self._kf_origins = np.full(int(config.keyframe_max), -1, dtype=np.int64)
        self._correct_counters = None
        # covisibility: its buffer and the pose on first use; the rows the last call found outside its table
        self._covis = None
        # estimate_exposure / apply_exposure: one buffer of 8-byte words -- record, sums, params -- and the pose, on first use
        self._exposure = None
        self.last_covis_outside = 0

    def _alloc_ws(self):
        if self.device.type != "cuda":
            return None
        n = _lib.load_library().gsl_map_ws_bytes(self.W, self.H)
        return torch.empty(n, dtype=torch.uint8, device=self.device)

    @property
    def points(self) -> Tensor:
        return self.means[: self.n_live]

    @property
    def point_colors(self) -> Tensor:
        return self.colors[: self.n_live]

    @property
    def survivors(self) -> Tensor:
        """int32: the old row of every row that was live after the last ``remove_seen_through`` or ``evict`` (empty before
        the first one); a view that the next call overwrites."""
        if self._free is None:
            return torch.zeros(0, dtype=torch.int32, device=self.device)
        return self._free["ids"][: self._n_survivors]

    def clear(self) -> None:
        self.n_live, self.full = 0, False
        self.frame_index, self.last_evicted = 0, 0
        self._view_rows = -1
        self._n_survivors = 0
        self._kf_made = 0
        self._n_inserts, self._last_origin = 0, -1
        self._kf_origins[:] = -1

    def _image(self, a, shape, what: str) -> Tensor:
        """a as a contiguous float32 tensor of that shape on the map's device, refused unless it has that many elements."""
        a = torch.as_tensor(a, dtype=torch.float32, device=self.device)
        if a.numel() != math.prod(shape):
            raise ValueError(f"{what} is {tuple(a.shape)}, the map was built for {shape}")
        return a.reshape(shape).contiguous()

    def _depth_image(self, depth) -> Tensor:
        return self._image(depth, (self.H, self.W), "depth")

    def _select_launch(self, depth: Tensor, render: Optional[Tensor], alphas: Optional[Tensor],
                       read_back: bool = True) -> Optional[int]:
        """The first entry point on the current stream; a frame that may not fit reads the pixels selected back here,
        its extra synchronisation."""
        assert depth.is_cuda, "GaussianMap.insert_frame: the map is grown by HIP kernels, no CPU path"
        lib, st, ptr, ws = _lib.load_library(), _lib.current_stream(), _lib.ptr, self._ws
        _lib.check(lib.gsl_map_select(ptr(render), ptr(alphas), ptr(depth), self.W, self.H, self.alpha_min, self.keep,
                                      ptr(self._counters), ptr(ws), ws.numel(), st), "gsl_map_select")
        return self._counters.tolist()[0] if read_back else None

    def _append_launch(self, depth: Tensor, rgb: Tensor, intr: Tuple[float, float, float, float], c2w: Tensor,
                       read_back: bool = True) -> Optional[int]:
        """The second entry point after ``_select_launch`` (the selection's workspace is untouched: an eviction in
        between has its own) and, for that frame, the read-back of the rows appended."""
        lib, st, ptr, ws = _lib.load_library(), _lib.current_stream(), _lib.ptr, self._ws
        _lib.check(lib.gsl_map_append(ptr(depth), ptr(rgb), self.W, self.H, *intr, ptr(c2w), ptr(self.means),
                                      ptr(self.colors), self.n_live, self.capacity, ptr(self._counters), ptr(ws),
                                      ws.numel(), st), "gsl_map_append")
        return self._counters.tolist()[1] if read_back else None

    def _launch(self, depth: Tensor, rgb: Tensor, intr: Tuple[float, float, float, float], c2w: Tensor,
                render: Optional[Tensor], alphas: Optional[Tensor]) -> Tuple[int, int]:
        """A frame with room: the two entry points and one read-back of (selected, appended)."""
        self._select_launch(depth, render, alphas, read_back=False)
        self._append_launch(depth, rgb, intr, c2w, read_back=False)
        selected, appended = self._counters.tolist()  # the frame's one synchronisation
        return selected, appended

    @torch.no_grad()
    def insert_frame(self, depth, rgb, K, c2w, render: Optional[Tensor] = None,
                     alphas: Optional[Tensor] = None, origin: Optional[int] = None) -> Tuple[int, int]:
        """depth [H,W] metres, rgb [H,W,3] in 0..255, K [3,3], c2w [4,4] the frame's pose in the world; render / alphas
        [H,W]: the map's expected depth (metres) and alpha at that pose -- both None: every pixel with a valid depth is
        new (the first frame).  Returns (pixels selected, rows appended); they differ when the map is full.  The rows
        appended are stamped with ``frame_index``.  ``MapConfig.evict``: a frame that may not fit (n_live + W * H above
        the capacity) reads its selection's count back before the append and, when it is short of room, first evicts
        that many rows plus ``evict_headroom`` (``evict``; ``last_evicted`` counts them).  ``MapConfig.refine``: the rows
        appended get the weight 1.  ``MapConfig.origins``: the rows appended get the origin ``origin`` -- the index of
        the frame in the caller's trajectory; None: the number of insert_frame calls since ``clear()`` -- which must be
        at least 0 and at least the origin of the insertion before (a ValueError before any launch).  Every removal
        compacts in map order and every append goes to the end, so ``origins[:n_live]`` is non-decreasing at all
        times, and the rows of the frames up to k are a prefix of the map (``rows_up_to``).  Without the option
        ``origin`` is not looked at."""
        if (render is None) != (alphas is None):
            raise ValueError("insert_frame: render and alphas come together (or neither, for the first frame)")
        if self.origins is not None:
            if origin is None:
                origin = self._n_inserts
            if isinstance(origin, bool) or not isinstance(origin, (int, np.integer)):
                raise ValueError(f"origin {origin!r}: a whole frame index")
            origin = int(origin)
            if not 0 <= origin < 2 ** 31 or origin < self._last_origin:
                raise ValueError(f"origin {origin}: at least 0 and at least the origin of the insertion before "
                                 f"({self._last_origin}): the origins are non-decreasing in map order")
        hw = (self.H, self.W)
        depth, rgb = self._depth_image(depth), self._image(torch.as_tensor(rgb)[..., :3], hw + (3,), "rgb")
        if render is not None:
            render, alphas = self._image(render, hw, "render"), self._image(alphas, hw, "alphas")
        intr, c2w = _intr_and_pose(K, c2w)
        c2w = c2w.to(device=self.device, dtype=torch.float32).contiguous()
        self.last_evicted = 0
        if self.cfg.evict and self.n_live + self.W * self.H > self.capacity:
            selected = self._select_launch(depth, render, alphas)
            short = selected - (self.capacity - self.n_live) + int(self.cfg.evict_headroom)
            if selected > 0 and short > 0:
                self.last_evicted = self.evict(short)[0]
            appended = self._append_launch(depth, rgb, intr, c2w)
        else:
            selected, appended = self._launch(depth, rgb, intr, c2w, render, alphas)
        if appended > 0:
            self.stamps[self.n_live:self.n_live + appended] = self.frame_index
            if self.weights is not None:
                self.weights[self.n_live:self.n_live + appended] = 1
            if self.origins is not None:
                self.origins[self.n_live:self.n_live + appended] = origin
        if self.origins is not None:
            self._last_origin = origin
        self._n_inserts += 1
        self.n_live += appended
        self.full = self.full or appended < selected
        return selected, appended

    # ---- the local map: the live rows in view from a pose (csrc/map_view.hip) ---------------------------------------
    def _view_buffers(self):
        if self._view is None:
            cap, dev, ws = self.capacity, self.device, []
            if dev.type == "cuda":
                n = _lib.load_library().gsl_map_view_ws_bytes(cap)
                ws = [torch.empty(n, dtype=torch.uint8, device=dev) for _ in range(2)]
            self._view = dict(means=torch.zeros(cap, 3, device=dev), colors=torch.zeros(cap, 3, device=dev),
                              ids=torch.zeros(cap, dtype=torch.int32, device=dev),
                              counters=torch.zeros(3, dtype=torch.int32, device=dev), ws=ws)
        return self._view

    def _view_launch(self, intr: Tuple[float, float, float, float], w2c: Tensor, guard_px: float, near: float,
                     far: float, check: bool) -> Tuple[int, int, int]:
        """check False: select the live rows into the first workspace and gather them into the working buffers; True:
        select into the second workspace against the ballots of the first, no gather.  The read-back of the counters
        (in view, in view and not in the first workspace's selection, gathered)."""
        assert self.means.is_cuda, "GaussianMap.select_view: the rows are selected by HIP kernels, no CPU path"
        lib, st, ptr, v = _lib.load_library(), _lib.current_stream(), _lib.ptr, self._view_buffers()
        ws, prev = (v["ws"][1], v["ws"][0]) if check else (v["ws"][0], None)
        _lib.check(lib.gsl_map_view_select(ptr(self.means), self.n_live, ptr(w2c), *intr, self.W, self.H, guard_px, near,
                                           far, ptr(prev), ptr(v["counters"]), ptr(ws), ws.numel(), st),
                   "gsl_map_view_select")
        if not check:
            _lib.check(lib.gsl_map_view_gather(ptr(self.means), ptr(self.colors), self.n_live, ptr(v["means"]),
                                               ptr(v["colors"]), ptr(v["ids"]), self.capacity, ptr(v["counters"]),
                                               ptr(ws), ws.numel(), st), "gsl_map_view_gather")
        in_view, fresh, gathered = v["counters"].tolist()  # the call's one synchronisation
        return in_view, fresh, gathered

    def _view_args(self, K, c2w):
        intr, c2w = _intr_and_pose(K, c2w)
        return intr, _world_to_camera(c2w).to(self.device).contiguous()

    # ---- occlusion culling of the local map: a z-buffer of the map's own rows (csrc/map_occl.hip) --------------------
    def occlusion_grid(self, guard_px: float) -> Tuple[int, int, int]:
        """(gi, CH, CW) of the z-buffer for this guard band and ``view_occlusion_cell_px``: the image widened by
        gi = ceil(guard_px) pixels, in cells."""
        cell = int(self.cfg.view_occlusion_cell_px)
        if not float(guard_px) >= 0.0 or not float(guard_px) < 2 ** 24:
            raise ValueError(f"guard_px {guard_px}: not negative, below 2^24")
        gi = int(math.ceil(np.float32(guard_px)))
        return gi, (self.H - 1 + 2 * gi) // cell + 1, (self.W - 1 + 2 * gi) // cell + 1

    def _occl_buffers(self):
        if self._occl is None:
            cap, dev, ws = self.capacity, self.device, []
            if dev.type == "cuda":
                n = _lib.load_library().gsl_map_occl_ws_bytes(cap)
                ws = [torch.empty(n, dtype=torch.uint8, device=dev) for _ in range(2)]
            self._occl = dict(counters=torch.zeros(4, dtype=torch.int32, device=dev), ws=ws, zbufs={})
        return self._occl

    def _occl_zbuf(self, guard_px: float) -> Tensor:
        """The z-buffer [CH, CW] of this guard band's grid (the uint32 keys as int32), allocated once per grid size."""
        _, ch, cw = self.occlusion_grid(guard_px)
        zbufs = self._occl_buffers()["zbufs"]
        if (ch, cw) not in zbufs:
            if ch * cw > 2 ** 26:
                raise ValueError(f"occlusion z-buffer of {ch} x {cw} cells: at most 2^26")
            zbufs[(ch, cw)] = torch.zeros(ch, cw, dtype=torch.int32, device=self.device)
        return zbufs[(ch, cw)]

    def _occl_depth_launch(self, intr: Tuple[float, float, float, float], w2c: Tensor, guard_px: float, near: float,
                           far: float) -> Tensor:
        """The z-buffer of the live rows from this pose; no read-back."""
        assert self.means.is_cuda, "GaussianMap.select_view: the rows are selected by HIP kernels, no CPU path"
        lib, st, ptr, zb = _lib.load_library(), _lib.current_stream(), _lib.ptr, self._occl_zbuf(guard_px)
        _lib.check(lib.gsl_map_occl_depth(ptr(self.means), self.n_live, ptr(w2c), *intr, self.W, self.H, guard_px,
                                          int(self.cfg.view_occlusion_cell_px), near, far, ptr(zb), 4 * zb.numel(), st),
                   "gsl_map_occl_depth")
        return zb

    def _occl_launch(self, intr: Tuple[float, float, float, float], w2c: Tensor, guard_px: float, near: float,
                     far: float, check: bool, rho: float) -> Tuple[int, int, int, int]:
        """``_view_launch`` with the occlusion rule: the z-buffer at this pose, the selection and, unless ``check``, the
        gather.  The read-back of the counters (selected, selected and not in the first workspace's selection, gathered,
        in the band and occluded)."""
        zb = self._occl_depth_launch(intr, w2c, guard_px, near, far)
        lib, st, ptr, v, o = _lib.load_library(), _lib.current_stream(), _lib.ptr, self._view_buffers(), self._occl
        ws, prev = (o["ws"][1], o["ws"][0]) if check else (o["ws"][0], None)
        keep = float(np.float32(1.0) - np.float32(rho))
        _lib.check(lib.gsl_map_occl_select(ptr(self.means), self.n_live, ptr(w2c), *intr, self.W, self.H, guard_px, near,
                                           far, int(self.cfg.view_occlusion_cell_px),
                                           int(self.cfg.view_occlusion_window), keep, ptr(zb), 4 * zb.numel(), ptr(prev),
                                           ptr(o["counters"]), ptr(ws), ws.numel(), st), "gsl_map_occl_select")
        if not check:
            _lib.check(lib.gsl_map_view_gather(ptr(self.means), ptr(self.colors), self.n_live, ptr(v["means"]),
                                               ptr(v["colors"]), ptr(v["ids"]), self.capacity, ptr(o["counters"]),
                                               ptr(ws), ws.numel(), st), "gsl_map_view_gather")
        selected, fresh, gathered, culled = o["counters"].tolist()  # the call's one synchronisation
        return selected, fresh, gathered, culled

    @torch.no_grad()
    def view_depth(self, K, c2w, guard_px: float, near: float, far: float) -> Tuple[Tensor, Tensor]:
        """The occlusion z-buffer of the live rows from the pose c2w, for tests and figures: (depth float32 [CH, CW],
        the nearest depth of the rows in each cell, inf where a cell is empty; the raw keys int32 [CH, CW], the uint32
        the kernel keeps -- 0 or the complement of the depth's bits -- reinterpreted).  Copies."""
        if self.n_live == 0:
            _, ch, cw = self.occlusion_grid(guard_px)
            return (torch.full((ch, cw), float("inf"), device=self.device),
                    torch.zeros(ch, cw, dtype=torch.int32, device=self.device))
        intr, w2c = self._view_args(K, c2w)
        raw = self._occl_depth_launch(intr, w2c, float(guard_px), float(near), float(far)).clone()
        depth = torch.where(raw == 0, torch.full_like(raw, float("inf"), dtype=torch.float32),
                            torch.bitwise_not(raw).view(torch.float32))
        return depth, raw

    @torch.no_grad()
    def select_view(self, K, c2w, guard_px: float, near: float, far: float,
                    occlusion_rho: Optional[float] = None) -> Tuple[Tensor, Tensor, Tensor, int]:
        """The live rows in view from the pose c2w [4,4] -- inside the image widened by guard_px on every side, between
        the depth planes (the rule: include/gsloc_hip.h) -- in map order.  Returns (points [n,3], colors [n,3],
        ids [n] int32, n): views of the prefix of capacity-sized working buffers that the next call overwrites.
        ``occlusion_rho``: of those rows, the ones that no nearer surface of the map hides (``MapConfig.
        view_occlusion_rho`` has the rule; the cell size and the window are the configuration's); ``last_view_culled``
        then counts the rows in the band that were left out, and is 0 without it."""
        if occlusion_rho is not None and not 0.0 < float(occlusion_rho) < 1.0:
            raise ValueError(f"occlusion_rho {occlusion_rho!r}: inside (0, 1)")
        v = self._view_buffers()
        n, culled = 0, 0
        if self.n_live > 0:
            intr, w2c = self._view_args(K, c2w)
            if occlusion_rho is None:
                n = self._view_launch(intr, w2c, float(guard_px), float(near), float(far), False)[2]
            else:
                _, _, n, culled = self._occl_launch(intr, w2c, float(guard_px), float(near), float(far), False,
                                                    float(occlusion_rho))
        self._view_rows, self._view_rho, self.last_view_culled = self.n_live, occlusion_rho, culled
        return v["means"][:n], v["colors"][:n], v["ids"][:n], n

    @torch.no_grad()
    def view_violations(self, K, c2w, near: float, far: float) -> int:
        """How many live rows are in view from c2w, the image widened by ``view_reach_px``, that the last select_view
        left out: 0 says that selection covers the view from c2w.  The rule is the one that select_view used: after one
        with ``occlusion_rho`` the z-buffer is built at c2w, with ``view_reach_px`` as guard, and the rows counted are
        those VISIBLE from there -- a row that parallax has uncovered counts, a row occluded from both poses does
        not."""
        if self._view_rows != self.n_live:
            raise RuntimeError("view_violations: no select_view of the rows that are live now")
        if self.n_live == 0:
            return 0
        intr, w2c = self._view_args(K, c2w)
        if self._view_rho is not None:
            return self._occl_launch(intr, w2c, float(self.cfg.view_reach_px), float(near), float(far), True,
                                     float(self._view_rho))[1]
        return self._view_launch(intr, w2c, float(self.cfg.view_reach_px), float(near), float(far), True)[1]

    # ---- free space: the live rows a depth frame sees through are removed (csrc/map_free.hip) ------------------------
    def _free_buffers(self):
        if self._free is None:
            cap, dev, ws = self.capacity, self.device, None
            if dev.type == "cuda":
                ws = torch.empty(_lib.load_library().gsl_map_view_ws_bytes(cap), dtype=torch.uint8, device=dev)
            self._free = dict(means=torch.zeros(cap, 3, device=dev), colors=torch.zeros(cap, 3, device=dev),
                              stamps=torch.zeros(cap, dtype=torch.int32, device=dev),
                              weights=None if self.weights is None else torch.zeros(cap, dtype=torch.int32, device=dev),
                              origins=None if self.origins is None else torch.zeros(cap, dtype=torch.int32, device=dev),
                              ids=torch.zeros(cap, dtype=torch.int32, device=dev),
                              counters=torch.zeros(3, dtype=torch.int32, device=dev), ws=ws)
        return self._free

    def _survivors_launch(self, counters: Tensor, ws: Tensor, stamps_early: bool, then=None) -> list:
        """What follows an operation's own selection of the rows that stay (their ballots in the head of ws, in the
        layout of gsl_map_view_select): their gather into the spare buffers (means, colours, old rows), the gather of
        their stamps, ``then()`` -- launches that work on the gathered rows -- and the read-back of the counters, the
        call's one synchronisation.  stamps_early: the stamps go before the read-back, every live row at most (the count
        is not known on the host yet, and the rows past it are never read); otherwise after it, the rows stored, and
        only when something goes -- the buffers will be swapped, the stamps follow their rows.  ``MapConfig.refine``:
        the weights follow them in the same way, by the same gather; ``MapConfig.origins``: and so do the origins (a
        fused voxel keeps the origin of the row that stays, the first in map order)."""
        lib, st, ptr, f = _lib.load_library(), _lib.current_stream(), _lib.ptr, self._free_buffers()

        def stamps(n):
            _lib.check(lib.gsl_map_gather_i32(ptr(self.stamps), self.n_live, ptr(f["ids"]), n, ptr(f["stamps"]), st),
                       "gsl_map_gather_i32")
            if self.weights is not None:
                _lib.check(lib.gsl_map_gather_i32(ptr(self.weights), self.n_live, ptr(f["ids"]), n, ptr(f["weights"]),
                                                  st), "gsl_map_gather_i32")
            if self.origins is not None:
                _lib.check(lib.gsl_map_gather_i32(ptr(self.origins), self.n_live, ptr(f["ids"]), n, ptr(f["origins"]),
                                                  st), "gsl_map_gather_i32")

        _lib.check(lib.gsl_map_view_gather(ptr(self.means), ptr(self.colors), self.n_live, ptr(f["means"]),
                                           ptr(f["colors"]), ptr(f["ids"]), self.capacity, ptr(counters), ptr(ws),
                                           ws.numel(), st), "gsl_map_view_gather")
        if stamps_early:
            stamps(self.n_live)
        if then is not None:
            then()
        out = counters.tolist()
        if not stamps_early and out[2] < self.n_live:
            stamps(out[2])
        return out

    def _keep_survivors(self, stay: int, gone: int, stored: int) -> Tuple[int, int]:
        """The end of a removal, from the counts its launches read back: ``survivors`` describes the rows that stay, and
        when something went the spare buffers, which hold them, become the map (a swap, not a copy).  (gone, kept)."""
        # the spare buffers hold the capacity: every row that stays was stored
        assert stored == stay == self.n_live - gone <= self.n_live, (stay, gone, stored, self.n_live)
        self._n_survivors = stay
        if gone > 0:
            f = self._free
            self.means, f["means"] = f["means"], self.means
            self.colors, f["colors"] = f["colors"], self.colors
            self.stamps, f["stamps"] = f["stamps"], self.stamps
            if self.weights is not None:
                self.weights, f["weights"] = f["weights"], self.weights
            if self.origins is not None:
                self.origins, f["origins"] = f["origins"], self.origins
            self.n_live = stay
            self._view_rows = -1  # the view ballots describe other rows
        return gone, stay

    def _free_launch(self, depth: Tensor, intr: Tuple[float, float, float, float], w2c: Tensor, keep: float,
                     window: int, near: float) -> Tuple[int, int]:
        """The rule over the live rows and ``_survivors_launch``; (rows that stay, rows stored)."""
        assert depth.is_cuda, "GaussianMap.remove_seen_through: the rows are judged and moved by HIP kernels, no CPU path"
        f = self._free_buffers()
        ws, ptr = f["ws"], _lib.ptr
        _lib.check(_lib.load_library().gsl_map_free_select(
            ptr(self.means), self.n_live, ptr(w2c), *intr, ptr(depth), self.W, self.H, keep, window, near,
            ptr(f["counters"]), ptr(ws), ws.numel(), _lib.current_stream()), "gsl_map_free_select")
        stay, _, stored = self._survivors_launch(f["counters"], ws, stamps_early=False)
        return stay, stored

    @torch.no_grad()
    def remove_seen_through(self, depth, K, c2w, near: float) -> Tuple[int, int]:
        """Removes the live rows that the depth frame [H,W] (metres) at the pose c2w [4,4] sees through (the rule:
        include/gsloc_hip.h, with ``free_rho`` and ``free_window_px``); the rows that stay keep their order.  Returns
        (removed, kept).  When something was removed the survivors were compacted into a spare pair of buffers that
        are ``means`` / ``colors`` from now on (a swap, not a copy -- compacting in place would let a workgroup
        overwrite rows another has not read yet): views taken from ``points`` / ``point_colors`` before the call are
        stale, ``survivors`` holds the old row of every live row, and the next ``view_violations`` needs a fresh
        ``select_view``.  When nothing was removed nothing changes."""
        if self._free_keep is None:
            raise RuntimeError("remove_seen_through: MapConfig.free_rho is None, the map only grows")
        if self.n_live == 0:
            return 0, 0
        depth = self._depth_image(depth)
        intr, w2c = self._view_args(K, c2w)
        stay, stored = self._free_launch(depth, intr, w2c, self._free_keep, int(self.cfg.free_window_px), float(near))
        return self._keep_survivors(stay, self.n_live - stay, stored)

    # ---- a bounded map: last-observed stamps, the least recently observed rows evicted (csrc/map_evict.hip) ---------
    def _observe_launch(self, depth: Tensor, intr: Tuple[float, float, float, float], w2c: Tensor, near: float,
                        far: float) -> None:
        assert depth.is_cuda, "GaussianMap.observe: the rows are stamped by a HIP kernel, no CPU path"
        lib, st, ptr = _lib.load_library(), _lib.current_stream(), _lib.ptr
        _lib.check(lib.gsl_map_observe(ptr(self.means), self.n_live, ptr(w2c), *intr, ptr(depth), self.W, self.H,
                                       self.keep, int(self.cfg.observe_window_px), float(self.cfg.view_reach_px), near,
                                       far, self.frame_index, ptr(self.stamps), st), "gsl_map_observe")

    @torch.no_grad()
    def observe(self, depth, K, c2w, near: float, far: float) -> None:
        """A new frame: ``frame_index`` goes up by one, and the live rows that the depth frame [H,W] (metres) at the pose
        c2w [4,4] observes (the rule: include/gsloc_hip.h, with ``depth_rho``, ``observe_window_px`` and
        ``view_reach_px``) are stamped with it.  No read-back."""
        self.frame_index += 1
        if self.n_live == 0:
            return
        depth = self._depth_image(depth)
        intr, w2c = self._view_args(K, c2w)
        self._observe_launch(depth, intr, w2c, float(near), float(far))

    def _evict_launch(self, need: int) -> Tuple[int, int, int]:
        """The selection over the stamps of the live rows and ``_survivors_launch``; (rows that stay, rows evicted, rows
        stored)."""
        assert self.means.is_cuda, "GaussianMap.evict: the rows are chosen and moved by HIP kernels, no CPU path"
        lib, f = _lib.load_library(), self._free_buffers()
        if self._evict_ws is None:
            self._evict_ws = torch.empty(lib.gsl_map_evict_ws_bytes(self.capacity), dtype=torch.uint8, device=self.device)
        ws = self._evict_ws
        _lib.check(lib.gsl_map_evict_select(_lib.ptr(self.stamps), self.n_live, self.frame_index,
                                            int(self.cfg.evict_min_age), need, _lib.ptr(f["counters"]), _lib.ptr(ws),
                                            ws.numel(), _lib.current_stream()), "gsl_map_evict_select")
        return tuple(self._survivors_launch(f["counters"], ws, stamps_early=True))

    @torch.no_grad()
    def evict(self, need: int) -> Tuple[int, int]:
        """Removes min(need, evictable) live rows -- evictable: last observed at least ``evict_min_age`` frames before
        ``frame_index`` -- the least recently observed first, in map order among rows of the same age (the rule:
        include/gsloc_hip.h); the rows that stay keep their order.  Returns (evicted, kept).  A swap as in
        ``remove_seen_through``: when something went, views taken before the call are stale, ``survivors`` holds the
        old row of every live row, and the next ``view_violations`` needs a fresh ``select_view``."""
        need = int(need)
        if need <= 0 or self.n_live == 0:
            return 0, self.n_live
        return self._keep_survivors(*self._evict_launch(need))

    # ---- a map with a resolution: the rows that share a voxel are fused into one (csrc/map_merge.hip) ----------------
    def _merge_launch(self) -> Tuple[int, int, int, int]:
        """The rule over the live rows and ``_survivors_launch``, with the fused rows written over the first row of
        their voxel in the spare buffers before the read-back; (rows that stay, rows removed, rows stored, the table's
        overflow flag)."""
        assert self.means.is_cuda, "GaussianMap.merge: the rows are fused and moved by HIP kernels, no CPU path"
        lib, st, ptr, f = _lib.load_library(), _lib.current_stream(), _lib.ptr, self._free_buffers()
        if self._merge is None:
            self._merge = dict(ws=torch.empty(lib.gsl_map_merge_ws_bytes(self.capacity), dtype=torch.uint8,
                                              device=self.device),
                               counters=torch.zeros(4, dtype=torch.int32, device=self.device))
        ws, counters = self._merge["ws"], self._merge["counters"]
        _lib.check(lib.gsl_map_merge_select(ptr(self.means), ptr(self.colors), ptr(self.stamps), self.n_live,
                                            self._merge_inv_h, self._merge_h, ptr(counters), ptr(ws), ws.numel(), st),
                   "gsl_map_merge_select")

        def apply():
            _lib.check(lib.gsl_map_merge_apply(ptr(f["ids"]), ptr(counters), self.n_live, ptr(f["means"]),
                                               ptr(f["colors"]), ptr(f["stamps"]), ptr(ws), ws.numel(), st),
                       "gsl_map_merge_apply")

        return tuple(self._survivors_launch(counters, ws, stamps_early=True, then=apply))

    @torch.no_grad()
    def merge(self) -> Tuple[int, int]:
        """Fuses the live rows that share a voxel of side ``merge_voxel`` (the rule: include/gsloc_hip.h): of the rows
        of a voxel the first in map order stays and becomes their mean position, mean colour and latest stamp, the
        others are removed; a row alone in its voxel, and a row with a NaN / inf or too distant mean, keeps every bit.
        The rows that stay keep their order.  Returns (removed, kept).  A swap as in ``remove_seen_through``: when
        something was removed, views taken before the call are stale, ``survivors`` holds the old row of every live
        row, and the next ``view_violations`` needs a fresh ``select_view``.  When nothing was removed nothing
        changes.  ``MapConfig.refine``: a fused row keeps the weight of the row it is kept at, the first of its voxel
        (the weights of the others are not summed: csrc/map_merge.hip knows nothing of them)."""
        if self._merge_h is None:
            raise RuntimeError("merge: MapConfig.merge_voxel is None, the map has no resolution")
        if self.n_live == 0:
            return 0, 0
        stay, removed, stored, overflow = self._merge_launch()
        if overflow != 0:
            raise RuntimeError("GaussianMap.merge: a row found no slot in the voxel table (gsl_map_merge_select)")
        return self._keep_survivors(stay, removed, stored)

    # ---- pose scores: how many live rows a depth frame confirms from each of a set of poses (csrc/map_score.hip) ----
    def _score_launch(self, depth: Tensor, intr: Tuple[float, float, float, float], w2c: Tensor, near: float,
                      n_rows: Optional[int] = None) -> np.ndarray:
        """w2c [k,4,4] float32 on the host.  The poses' copy to the device, the entry point (which zeroes the counts) and
        the read-back of int64 [k,3]: (tested, agree, front) per pose.  n_rows: the first rows of the map that are
        judged (None: the live ones)."""
        n_rows = self.n_live if n_rows is None else int(n_rows)
        assert depth.is_cuda, "GaussianMap.score_poses: the rows are judged and counted by a HIP kernel, no CPU path"
        lib, st, ptr = _lib.load_library(), _lib.current_stream(), _lib.ptr
        if self._score is None:
            self._score = dict(counts=torch.empty(SCORE_MAX_POSES, 3, dtype=torch.int32, device=self.device),
                               poses=torch.empty(SCORE_MAX_POSES, 16, device=self.device))
        k, s = w2c.shape[0], self._score
        s["poses"][:k].copy_(w2c.reshape(k, 16))
        _lib.check(lib.gsl_map_score(ptr(self.means), n_rows, ptr(s["poses"]), k, *intr, ptr(depth), self.W, self.H,
                                     self.keep, self.beyond, near, ptr(s["counts"]), st), "gsl_map_score")
        return s["counts"][:k].cpu().numpy().astype(np.int64)  # the call's one synchronisation

    @torch.no_grad()
    def score_poses(self, depth, K, c2ws, near: float, rows: Optional[int] = None) -> np.ndarray:
        """How the depth frame [H,W] (metres) agrees with the live rows from each of the poses c2ws [k,4,4] (a tensor,
        or a sequence of [4,4] poses; k <= 64).  Returns int64 [k,3]: per pose the rows TESTED (in the image, beyond the
        near plane, their own pixel has a depth), those that AGREE (within ``depth_rho`` of that depth either way) and
        those in FRONT of it (the rule: include/gsloc_hip.h); tested - agree - front lie behind, where a frame that
        sees a nearer surface says nothing against them.  One launch for all poses, one read-back; an empty map gives
        zeros without a launch.  rows: only the first that many rows of the map are judged (``loop_constraint``; None:
        every live row)."""
        rows = self._prefix(rows)
        poses = [torch.as_tensor(c) for c in c2ws]
        for c in poses:
            if c.shape != (4, 4):
                raise ValueError(f"a pose is {tuple(c.shape)}, not (4, 4)")
        if len(poses) > SCORE_MAX_POSES:
            raise ValueError(f"{len(poses)} poses: one call scores at most {SCORE_MAX_POSES}")
        if (self.n_live if rows is None else rows) == 0 or not poses:
            return np.zeros((len(poses), 3), dtype=np.int64)
        depth = self._depth_image(depth)
        intr, _ = _intr_and_pose(K, poses[0])
        w2c = _world_to_camera(torch.stack([c.detach().cpu().double() for c in poses]))
        if rows is None:
            return self._score_launch(depth, intr, w2c, float(near))
        return self._score_launch(depth, intr, w2c, float(near), n_rows=rows)

    def _prefix(self, rows: Optional[int]) -> Optional[int]:
        """rows as a count of leading live rows (None stays None), refused outside 0 .. n_live."""
        if rows is None:
            return None
        if isinstance(rows, bool) or not isinstance(rows, (int, np.integer)) or not 0 <= int(rows) <= self.n_live:
            raise ValueError(f"rows {rows!r}: a whole number of leading rows, 0 .. {self.n_live}")
        return int(rows)

    # ---- pose information: the normal equations of a pose from the rows against a depth frame (csrc/map_info.hip) ------
    def _info_launch(self, depth: Tensor, intr: Tuple[float, float, float, float], w2c: Tensor, keep: float,
                     beyond: float, kappa: float, near: float) -> np.ndarray:
        """w2c [4,4] float32 on the device.  The entry point (which zeroes the sums) and the read-back of int64 [30], the
        call's one synchronisation."""
        assert depth.is_cuda, "GaussianMap.pose_information: the rows are judged and summed by a HIP kernel, no CPU path"
        lib, st, ptr = _lib.load_library(), _lib.current_stream(), _lib.ptr
        if self._info is None:
            self._info = torch.empty(INFO_VALUES, dtype=torch.int64, device=self.device)
        _lib.check(lib.gsl_map_pose_info(ptr(self.means), self.n_live, ptr(w2c), *intr, ptr(depth), self.W, self.H, keep,
                                         beyond, kappa, near, ptr(self._info), st), "gsl_map_pose_info")
        return self._info.cpu().numpy()

    # ---- the photometric term of those normal equations (csrc/map_photo.hip) -------------------------------------------
    def _intensity_launch(self, rgb: Tensor) -> Tensor:
        """rgb [H,W,3] float32 on the device -> a new float32 [H,W]: one kernel, no synchronisation."""
        assert rgb.is_cuda, "GaussianMap.intensity: the image is made by a HIP kernel, no CPU path"
        lib, st, ptr = _lib.load_library(), _lib.current_stream(), _lib.ptr
        out = torch.empty(self.H, self.W, device=self.device)
        _lib.check(lib.gsl_map_photo_intensity(ptr(rgb), self.W, self.H, ptr(out), st), "gsl_map_photo_intensity")
        return out

    @torch.no_grad()
    def intensity(self, rgb) -> Tensor:
        """The intensity image [H,W] float32, 0 .. 1, of a frame's rgb [H,W,3] in 0 .. 255 -- ((0.299 R + 0.587 G) +
        0.114 B) / 255 in float32 -- on the map's device: what ``pose_information``, ``align_pose``, ``align_poses`` and
        ``loop_constraint`` take as ``intensity``.  One kernel; make it once per frame."""
        return self._intensity_launch(self._image(rgb, (self.H, self.W, 3), "rgb"))

    def _photo_params(self, intensity, photo_scale, photo_max_residual):
        """None without an intensity image; otherwise (the image [H,W] float32 on the device, photo_scale,
        photo_max_residual as float32 values) with the configuration's values where None is given, checked."""
        if intensity is None:
            if photo_scale is not None or photo_max_residual is not None:
                raise ValueError("photo_scale / photo_max_residual belong to a photometric term: they need intensity")
            return None
        scale = self.cfg.photo_scale if photo_scale is None else photo_scale
        if scale is None:
            raise ValueError("photo_scale: intensity is given and neither the call nor MapConfig sets the scale")
        scale = float(scale)
        if not 0.0 <= scale <= INFO_PHOTO_MAX_SCALE:
            raise ValueError(f"photo_scale {scale!r}: metres per unit of intensity, inside [0, {INFO_PHOTO_MAX_SCALE:g}]")
        rmax = float(self.cfg.photo_max_residual if photo_max_residual is None else photo_max_residual)
        if not 0.0 <= rmax <= 1.0:
            raise ValueError(f"photo_max_residual {rmax!r}: an intensity difference, inside [0, 1]")
        return (self._image(intensity, (self.H, self.W), "intensity"), float(np.float32(scale)), float(np.float32(rmax)))

    def _info_photo_launch(self, depth: Tensor, intr: Tuple[float, float, float, float], w2c: Tensor, keep: float,
                           beyond: float, kappa: float, near: float, photo) -> Tuple[np.ndarray, np.ndarray]:
        """``_info_launch`` with the photometric term, photo = (intensity, scale, max residual): the entry point (which
        zeroes the sums and the two extra words) and the read-back of (int64 [30], int64 [2]), the call's one
        synchronisation."""
        assert depth.is_cuda, "GaussianMap.pose_information: the rows are judged and summed by a HIP kernel, no CPU path"
        lib, st, ptr = _lib.load_library(), _lib.current_stream(), _lib.ptr
        if self._info_photo is None:
            self._info_photo = torch.empty(INFO_VALUES + 2, dtype=torch.int64, device=self.device)
        image, scale, rmax = photo
        out = self._info_photo.data_ptr()
        _lib.check(lib.gsl_map_pose_info_photo(ptr(self.means), self.n_live, ptr(w2c), *intr, ptr(depth), self.W, self.H,
                                               keep, beyond, kappa, near, out, ptr(self.colors), ptr(image), scale, rmax,
                                               out + 8 * INFO_VALUES, st), "gsl_map_pose_info_photo")
        host = self._info_photo.cpu().numpy()
        return host[:INFO_VALUES].copy(), host[INFO_VALUES:].copy()

    @torch.no_grad()
    def pose_information(self, depth, K, c2w, near_plane: float, rho: Optional[float] = None,
                         kappa: Optional[float] = None, intensity=None, photo_scale: Optional[float] = None,
                         photo_max_residual: Optional[float] = None) -> PoseInformation:
        """How well the depth frame [H,W] (metres) constrains the pose c2w [4,4]: the point-to-plane normal equations of
        a small move of the camera, summed over the live rows that project onto an inner pixel beyond ``near_plane``,
        agree with its depth within ``rho`` (None: ``info_rho``, and ``depth_rho`` when that is None) as do its four
        neighbours, and whose patch is planar within ``kappa`` (None: ``info_kappa``) -- the rule: include/gsloc_hip.h.
        Changes nothing in the map.  One zeroing launch, one kernel, one read-back; an empty map gives zeros (weak)
        without a launch.  intensity: None, or the frame's intensity image (``intensity(rgb)``): every used row then
        also gives a photometric equation from its colour, ``photo_scale`` metres per unit of intensity (None:
        ``MapConfig.photo_scale``) where it misses the image by at most ``photo_max_residual`` (None: the
        configuration's), summed into the same H, g and rss (csrc/map_photo.hip); ``photo_used`` and ``photo_rss``
        report its share.  One more zeroing launch."""
        photo = self._photo_params(intensity, photo_scale, photo_max_residual)
        min_eig = INFO_MIN_EIG if self.cfg.info_min_eig is None else float(self.cfg.info_min_eig)
        if rho is None:
            rho = self.cfg.depth_rho if self.cfg.info_rho is None else self.cfg.info_rho
        if not 0.0 <= rho < 1.0:
            raise ValueError(f"rho {rho!r}: a fraction of the observed depth, inside [0, 1)")
        kappa = float(self.cfg.info_kappa if kappa is None else kappa)
        if not (math.isfinite(kappa) and kappa >= 0.0):
            raise ValueError(f"kappa {kappa!r}: a fraction of the inverse depth, finite and not negative")
        depth = self._depth_image(depth)
        intr, c2w = _intr_and_pose(K, c2w)
        if self.n_live == 0:
            return PoseInformation(np.zeros((6, 6)), np.zeros(6), 0.0, 0, 0, min_eig)
        keep, beyond = float(np.float32(1.0) - np.float32(rho)), float(np.float32(1.0) + np.float32(rho))
        w2c = _world_to_camera(c2w).to(self.device).contiguous()
        if photo is not None:
            sums, extra = self._info_photo_launch(depth, intr, w2c, keep, beyond, float(np.float32(kappa)),
                                                  float(near_plane), photo)
            return information_from_sums(sums, min_eig, extra)
        sums = self._info_launch(depth, intr, w2c, keep, beyond, float(np.float32(kappa)), float(near_plane))
        return information_from_sums(sums, min_eig)

    # ---- the image pyramid of a frame, for coarse-to-fine alignment (csrc/map_pyramid.hip) ----------------------------
    def _pyramid_launch(self, depth: Tensor, image: Optional[Tensor], levels: int, keep: float):
        """depth [H,W] and, or None, image [H,W] float32 on the device -> (packed levels 1 .. levels of the depth, of the
        image or None): two new buffers, one kernel, no synchronisation."""
        assert depth.is_cuda, "GaussianMap.pyramid: the levels are made by a HIP kernel, no CPU path"
        lib, st, ptr = _lib.load_library(), _lib.current_stream(), _lib.ptr
        n = int(lib.gsl_map_pyramid_floats(self.W, self.H, levels))
        depth_out = torch.empty(n, device=self.device)
        image_out = None if image is None else torch.empty(n, device=self.device)
        _lib.check(lib.gsl_map_pyramid(ptr(depth), ptr(image), self.W, self.H, levels, keep, ptr(depth_out),
                                       ptr(image_out), st), "gsl_map_pyramid")
        return depth_out, image_out

    def _pyramid_keep(self, rho, align_rho=None) -> float:
        """1 - rho_p as the float32 value the kernel is given: rho, else ``pyramid_rho``, else the alignment's rho
        (align_rho when a call resolved it, else ``align_rho``, and ``depth_rho`` when that is None)."""
        if rho is None:
            rho = self.cfg.pyramid_rho
        if rho is None:
            rho = align_rho
        if rho is None:
            rho = self.cfg.depth_rho if self.cfg.align_rho is None else self.cfg.align_rho
        if not 0.0 <= rho < 1.0:
            raise ValueError(f"rho {rho!r}: a fraction of the largest depth of a block, inside [0, 1)")
        return float(np.float32(1.0) - np.float32(rho))

    @torch.no_grad()
    def pyramid(self, depth, levels: int, intensity=None, rho: Optional[float] = None, K=None) -> FramePyramid:
        """The image pyramid of a frame: its depth [H,W] (metres) and, when given, its intensity image [H,W]
        (``intensity(rgb)``) halved ``levels`` times (1 .. 4; the coarsest level at least 4 x 4).  A coarse depth is the
        inverse of the mean inverse depth of its 2 x 2 block -- exact on a plane -- where all four are valid and within
        ``rho`` of the largest (None: ``pyramid_rho``, and the alignment's rho when that is None), otherwise 0; a coarse
        intensity is the mean of its block (the rule: include/gsloc_hip.h).  K: the frame's intrinsics, for
        ``FramePyramid.intrs``.  What ``align_pose``, ``align_poses`` and ``loop_constraint`` take as ``pyramid``: build
        it once per frame.  One kernel, no synchronisation."""
        pyramid_sizes(self.W, self.H, levels)  # refuses what the entry point would
        levels = int(levels)
        keep = self._pyramid_keep(rho)
        depth = self._depth_image(depth)
        image = None if intensity is None else self._image(intensity, (self.H, self.W), "intensity")
        out = self._build_pyramid(depth, image, levels, keep)
        if K is not None:
            out.intrs = pyramid_intrinsics(_intr_and_pose(K, torch.eye(4))[0], levels)
        return out

    def _build_pyramid(self, depth: Tensor, image: Optional[Tensor], levels: int, keep: float) -> FramePyramid:
        """The launch and the per-level views into its two packed buffers, level 0 the inputs themselves."""
        sizes = pyramid_sizes(self.W, self.H, levels)
        depth_out, image_out = self._pyramid_launch(depth, image, levels, keep)
        depths, images, at = [depth], None if image is None else [image], 0
        for w, h in sizes[1:]:
            depths.append(depth_out[at:at + w * h].view(h, w))
            if image is not None:
                images.append(image_out[at:at + w * h].view(h, w))
            at += w * h
        return FramePyramid(levels, depths, images, sizes, keep)

    # ---- exposure compensation: an affine brightness model of a frame against the map (csrc/map_exposure.hip) ---------
    def _exposure_buffers(self):
        """words int64: record [4][6], sums [7], then params as four float32 in two words; the start pose."""
        if self._exposure is None:
            n = EXPOSURE_MAX_PASSES * EXPOSURE_RECORD_WORDS + EXPOSURE_VALUES + 2
            self._exposure = dict(words=torch.zeros(n, dtype=torch.int64, device=self.device),
                                  w2c=torch.empty(16, device=self.device))
            self._exposure["params"] = self._exposure["words"][n - 2:].view(torch.float32)
            self._exposure["params"].copy_(torch.tensor([1.0, 0.0, 0.0, 0.0]))
        return self._exposure

    def _exposure_params(self, rho, max_residual, saturation, passes, min_used, gain, max_offset, min_var):
        """The keyword arguments of ``estimate_exposure`` with the configuration's values where None is given, checked, in
        the units of the entry point: (keep, beyond, sat_lo, sat_hi, max_residual, passes, min_used, gain_min, gain_max,
        offset_max, min_var)."""
        cfg = self.cfg
        if rho is None:
            rho = cfg.exposure_rho
        if rho is None:
            rho = 0.05 if cfg.align_rho is None else cfg.align_rho
        if not 0.0 <= rho < 1.0:
            raise ValueError(f"rho {rho!r}: a fraction of the observed depth, inside [0, 1)")
        rmax = float(cfg.exposure_max_residual if max_residual is None else max_residual)
        if not 0.0 <= rmax <= 1.0:
            raise ValueError(f"max_residual {rmax!r}: an intensity difference, inside [0, 1]")
        lo, hi = _exposure_pair(cfg.exposure_saturation if saturation is None else tuple(saturation), "exposure_saturation")
        g_lo, g_hi = _exposure_pair(cfg.exposure_gain if gain is None else tuple(gain), "exposure_gain")
        passes = cfg.exposure_passes if passes is None else passes
        if isinstance(passes, bool) or not isinstance(passes, (int, np.integer)) or not 1 <= passes <= EXPOSURE_MAX_PASSES:
            raise ValueError(f"passes {passes!r}: a whole number of passes, 1 .. {EXPOSURE_MAX_PASSES}")
        min_used = int(cfg.exposure_min_used if min_used is None else min_used)
        if min_used < 1:
            raise ValueError(f"min_used {min_used!r}: at least 1 row")
        max_offset = float(cfg.exposure_max_offset if max_offset is None else max_offset)
        min_var = float(cfg.exposure_min_var if min_var is None else min_var)
        if not (math.isfinite(max_offset) and max_offset >= 0.0 and math.isfinite(min_var) and min_var >= 0.0):
            raise ValueError(f"max_offset / min_var {max_offset!r} / {min_var!r}: finite and not negative")
        keep, beyond = float(np.float32(1.0) - np.float32(rho)), float(np.float32(1.0) + np.float32(rho))
        lo32, hi32 = float(np.float32(lo)), float(np.float32(hi))
        if not 0.0 <= lo32 < hi32 <= 1.0:
            raise ValueError(f"saturation {(lo, hi)!r}: not a range as float32")
        return (keep, beyond, lo32, hi32, float(np.float32(rmax)), int(passes), min_used, g_lo, g_hi, max_offset, min_var)

    def _exposure_launch(self, depth: Tensor, image: Tensor, intr: Tuple[float, float, float, float], w2c: Tensor,
                         near: float, params) -> np.ndarray:
        """w2c [4,4] float32 on the host.  Its copy to the device, the entry point and the read-back of the one buffer,
        the call's one synchronisation: the int64 words (record, sums, params)."""
        assert depth.is_cuda, "GaussianMap.estimate_exposure: the rows are summed and solved by HIP kernels, no CPU path"
        lib, st, ptr = _lib.load_library(), _lib.current_stream(), _lib.ptr
        e = self._exposure_buffers()
        keep, beyond, lo, hi, rmax, passes, min_used, g_lo, g_hi, max_offset, min_var = params
        e["w2c"].copy_(w2c.reshape(16))
        base, n_rec = e["words"].data_ptr(), EXPOSURE_MAX_PASSES * EXPOSURE_RECORD_WORDS
        _lib.check(lib.gsl_map_exposure_estimate(ptr(self.means), ptr(self.colors), self.n_live, ptr(e["w2c"]), *intr,
                                                 ptr(depth), ptr(image), self.W, self.H, keep, beyond, near, lo, hi, rmax,
                                                 passes, min_used, g_lo, g_hi, max_offset, min_var, base + 8 * n_rec,
                                                 base + 8 * (n_rec + EXPOSURE_VALUES), base, st),
                   "gsl_map_exposure_estimate")
        return e["words"].cpu().numpy()

    @torch.no_grad()
    def estimate_exposure(self, depth, K, c2w, near_plane: float, rgb=None, intensity=None, rho: Optional[float] = None,
                          max_residual: Optional[float] = None, saturation=None, passes: Optional[int] = None,
                          min_used: Optional[int] = None, gain=None, max_offset: Optional[float] = None,
                          min_var: Optional[float] = None) -> Exposure:
        """The exposure of a frame against the map: gain and offset with gain * Y_frame + offset ~ Y_row over the live
        rows that the frame at c2w [4,4] sees -- a row projects beyond ``near_plane`` onto a pixel whose depth [H,W]
        (metres) is within ``rho`` of its own -- whose colour's intensity and the frame's at that pixel both lie inside
        ``saturation``, by ``passes`` least-squares passes, the later ones without the rows that miss by more than
        ``max_residual`` (None: the ``exposure_*`` fields of the configuration; the rule: include/gsloc_hip.h).  The
        frame is given as ``rgb`` [H,W,3] in 0 .. 255 (its intensity image is made here, one more kernel) or as
        ``intensity`` [H,W] (``intensity(rgb)``), one of the two.  Changes nothing in the map.  One fixed sequence of
        1 + 3 ``passes`` launches, one read-back; the pair stays on the device for ``apply_exposure(rgb)``.  An empty
        map gives the identity with status FEW and no launch."""
        if (rgb is None) == (intensity is None):
            raise ValueError("estimate_exposure takes the frame as rgb or as intensity, one of the two")
        params = self._exposure_params(rho, max_residual, saturation, passes, min_used, gain, max_offset, min_var)
        depth = self._depth_image(depth)
        if rgb is not None:
            rgb = self._image(rgb, (self.H, self.W, 3), "rgb")
        else:
            intensity = self._image(intensity, (self.H, self.W), "intensity")
        intr, c2w = _intr_and_pose(K, c2w)
        if self.n_live == 0:
            if self._exposure is not None:
                self._exposure["params"].copy_(torch.tensor([1.0, 0.0, 0.0, 0.0]))
            return Exposure(1.0, 0.0, "FEW", 0, 0, 0.0, [])
        image = self._intensity_launch(rgb) if rgb is not None else intensity
        host = self._exposure_launch(depth, image, intr, _world_to_camera(c2w).contiguous(), float(near_plane), params)
        return self._exposure_of(host, params[5])

    def _exposure_of(self, host: np.ndarray, passes: int) -> Exposure:
        """The ``Exposure`` of what a launch read back."""
        n_rec = EXPOSURE_MAX_PASSES * EXPOSURE_RECORD_WORDS
        rec = host[:passes * EXPOSURE_RECORD_WORDS].reshape(passes, EXPOSURE_RECORD_WORDS)
        sol = rec[:, 3:].copy().view(np.float64)
        pair = host[n_rec + EXPOSURE_VALUES:].copy().view(np.float32)
        history = [(EXPOSURE_STATUS[int(r[0])], int(r[1]), int(r[2]), float(x[0]), float(x[1]), float(x[2]))
                   for r, x in zip(rec, sol)]
        last = history[-1]
        return Exposure(float(pair[0]), float(pair[1]), last[0], last[1], last[2], last[5], history)

    @torch.no_grad()
    def apply_exposure(self, rgb, exposure=None) -> Tensor:
        """rgb [H,W,3] in 0 .. 255 corrected by an exposure: a new float32 [H,W,3] on the map's device, gain * rgb + 255 *
        offset clipped to 0 .. 255 -- its intensity image is gain * Y + offset.  exposure: None, the pair the last
        ``estimate_exposure`` left on the device (no read-back; the identity before the first); an ``Exposure`` or a
        (gain, offset) pair, uploaded.  One kernel, no synchronisation."""
        rgb = self._image(rgb, (self.H, self.W, 3), "rgb")
        if exposure is not None:
            pair = (exposure.gain, exposure.offset) if isinstance(exposure, Exposure) else tuple(exposure)
            if len(pair) != 2 or not all(math.isfinite(float(a)) for a in pair):
                raise ValueError(f"exposure {exposure!r}: an Exposure or a finite (gain, offset) pair")
            b = np.float32(pair[1])
            pair = torch.from_numpy(np.array([np.float32(pair[0]), b, b * np.float32(255.0), 0.0], np.float32))
        assert rgb.is_cuda, "GaussianMap.apply_exposure: the image is corrected by a HIP kernel, no CPU path"
        lib, st, ptr = _lib.load_library(), _lib.current_stream(), _lib.ptr
        e = self._exposure_buffers()
        params = e["params"] if exposure is None else pair.to(self.device)
        out = torch.empty(self.H, self.W, 3, device=self.device)
        _lib.check(lib.gsl_map_exposure_apply(ptr(rgb), self.W, self.H, ptr(params), ptr(out), st),
                   "gsl_map_exposure_apply")
        return out

    def _levels_params(self, levels, level_steps, steps: int):
        """The ``levels`` / ``level_steps`` arguments of ``align_pose`` / ``align_poses`` with their defaults filled in
        and checked: (levels, 0 for today's single level; the steps of a coarse level)."""
        if levels is None:
            levels = self.cfg.align_levels
        if isinstance(levels, bool) or not isinstance(levels, (int, np.integer)) or not 0 <= int(levels) <= PYRAMID_MAX_LEVELS:
            raise ValueError(f"levels {levels!r}: a whole number of pyramid levels, 0 .. {PYRAMID_MAX_LEVELS}")
        levels = int(levels)
        if levels > 0:
            pyramid_sizes(self.W, self.H, levels)
        if level_steps is None:
            level_steps = self.cfg.align_level_steps
        level_steps = steps if level_steps is None else level_steps
        if (isinstance(level_steps, bool) or not isinstance(level_steps, (int, np.integer))
                or not 1 <= int(level_steps) <= ALIGN_MAX_STEPS):
            raise ValueError(f"level_steps {level_steps!r}: a whole number of iterations, 1 .. {ALIGN_MAX_STEPS}")
        return levels, int(level_steps)

    def _level_frames(self, depth: Tensor, intr, photo, levels: int, pyramid: Optional[FramePyramid], keep: float) -> list:
        """Per level from ``levels`` down to 0 what an alignment entry point is given there: (depth image, (W, H),
        intrinsics, photo or None).  pyramid: a prebuilt one of this frame (at least ``levels`` levels, with intensities
        when photo is given), or None: built here, one launch."""
        if pyramid is None:
            pyramid = self._build_pyramid(depth, None if photo is None else photo[0], levels, keep)
        elif not isinstance(pyramid, FramePyramid) or pyramid.levels < levels or pyramid.sizes[0] != (self.W, self.H):
            raise ValueError(f"pyramid: a FramePyramid of this map's {self.W} x {self.H} frames with at least {levels} "
                             "levels")
        elif photo is not None and pyramid.intensities is None:
            raise ValueError("pyramid: it holds no intensities, and the call has a photometric term")
        sizes, depths, images = pyramid.sizes, pyramid.depths, pyramid.intensities
        intrs = pyramid_intrinsics(intr, levels)
        return [(depth if l == 0 else depths[l], sizes[l], intrs[l],
                 None if photo is None else ((photo[0] if l == 0 else images[l]), photo[1], photo[2]))
                for l in range(levels, -1, -1)]

    def _align_levels_launch(self, frames: list, w2c: Tensor, keep: float, beyond: float, kappa: float, near: float,
                             steps: int, level_steps: int, damping: float, min_used: int, max_rot: float,
                             max_trans: float, eps_rot: float, eps_trans: float, n_rows: Optional[int] = None) -> list:
        """``_align_launch`` once per level of frames (``_level_frames``: coarse to fine), level_steps iterations at the
        coarse levels and steps at level 0.  Every level has its own section of one buffer of 8-byte words, laid out as
        ``_align_launch``'s, and its own start pose; a level's working pose is copied on the device into the next
        level's start (the entry points forbid an overlap), and nothing is read back in between: the call's one
        synchronisation is the read-back of the whole buffer at the end.  Returns ``_align_launch``'s tuple per level."""
        assert frames[0][0].is_cuda, "GaussianMap.align_pose: the pose is aligned by HIP kernels, no CPU path"
        lib, st, ptr = _lib.load_library(), _lib.current_stream(), _lib.ptr
        n_state, n_hist = ALIGN_STATE_WORDS, ALIGN_MAX_STEPS * ALIGN_ROW_WORDS
        section, n = n_state + n_hist + 8 + INFO_VALUES, len(frames)
        if n not in self._align_levels:
            self._align_levels[n] = dict(words=torch.zeros(n * section, dtype=torch.int64, device=self.device),
                                         start=torch.empty(n, 16, device=self.device))
        a = self._align_levels[n]
        n_rows = self.n_live if n_rows is None else int(n_rows)
        words, start = a["words"], a["start"]
        work = words.view(torch.float32).view(n, 2 * section)[:, 2 * (n_state + n_hist):2 * (n_state + n_hist) + 16]
        start[0].copy_(w2c.reshape(16))
        for j, (depth, (w, h), intr, photo) in enumerate(frames):
            if j > 0:
                start[j].copy_(work[j - 1])  # device to device, on the stream: the next level starts where this one stood
            base = words.data_ptr() + 8 * j * section
            args = (ptr(self.means), n_rows, ptr(start[j]), *intr, ptr(depth), w, h, keep, beyond, kappa, near,
                    steps if j == n - 1 else level_steps, damping, min_used, max_rot, max_trans, eps_rot, eps_trans,
                    base + 8 * (n_state + n_hist + 8), base + 8 * (n_state + n_hist), base, base + 8 * n_state)
            if photo is None:
                _lib.check(lib.gsl_map_pose_align(*args, st), "gsl_map_pose_align")
            else:
                _lib.check(lib.gsl_map_pose_align_photo(*args, ptr(self.colors), ptr(photo[0]), photo[1], photo[2], st),
                           "gsl_map_pose_align_photo")
        host = words.cpu().numpy().reshape(n, section)
        out = []
        for j in range(n):
            taken = steps if j == n - 1 else level_steps
            hist = host[j, n_state:n_state + taken * ALIGN_ROW_WORDS].reshape(taken, ALIGN_ROW_WORDS)
            out.append((host[j, :12].view(np.float64).reshape(3, 4).copy(),
                        host[j, n_state + n_hist:n_state + n_hist + 8].view(np.float32).reshape(4, 4).copy(),
                        int(host[j, 12]), hist[:, :4].copy(), hist[:, 4:].copy().view(np.float64)))
        return out

    def _align_batch_levels_launch(self, frames: list, w2c: Tensor, keep: float, beyond: float, kappa: float,
                                   near: float, steps: int, level_steps: int, damping: float, min_used: int,
                                   max_rot: float, max_trans: float, eps_rot: float, eps_trans: float,
                                   n_rows: Optional[int] = None) -> list:
        """``_align_batch_launch`` once per level of frames, as ``_align_levels_launch`` does it for one pose: the k <=
        16 working poses of a level are copied on the device into the next level's starts, one read-back at the end.
        Returns per level ``_align_batch_launch``'s list."""
        assert frames[0][0].is_cuda, "GaussianMap.align_poses: the poses are aligned by HIP kernels, no CPU path"
        lib, st, ptr = _lib.load_library(), _lib.current_stream(), _lib.ptr
        cap, k, n = ALIGN_BATCH_MAX_POSES, int(w2c.shape[0]), len(frames)
        at_state, at_hist = 0, cap * ALIGN_STATE_WORDS
        at_work = at_hist + cap * ALIGN_MAX_STEPS * ALIGN_ROW_WORDS
        at_sums = at_work + cap * 8
        section = at_sums + cap * INFO_VALUES
        if n not in self._align_batch_levels:
            self._align_batch_levels[n] = dict(words=torch.zeros(n * section, dtype=torch.int64, device=self.device),
                                               start=torch.empty(n, cap, 16, device=self.device))
        a = self._align_batch_levels[n]
        n_rows = self.n_live if n_rows is None else int(n_rows)
        words, start = a["words"], a["start"]
        work = words.view(torch.float32).view(n, 2 * section)[:, 2 * at_work:2 * at_work + 16 * cap].view(n, cap, 16)
        start[0, :k].copy_(w2c.reshape(k, 16))
        for j, (depth, (w, h), intr, photo) in enumerate(frames):
            if j > 0:
                start[j, :k].copy_(work[j - 1, :k])
            base = words.data_ptr() + 8 * j * section
            args = (ptr(self.means), n_rows, ptr(start[j]), k, *intr, ptr(depth), w, h, keep, beyond, kappa, near,
                    steps if j == n - 1 else level_steps, damping, min_used, max_rot, max_trans, eps_rot, eps_trans,
                    base + 8 * at_sums, base + 8 * at_work, base + 8 * at_state, base + 8 * at_hist)
            if photo is None:
                _lib.check(lib.gsl_map_pose_align_batch(*args, st), "gsl_map_pose_align_batch")
            else:
                _lib.check(lib.gsl_map_pose_align_batch_photo(*args, ptr(self.colors), ptr(photo[0]), photo[1], photo[2],
                                                              st), "gsl_map_pose_align_batch_photo")
        host = words.cpu().numpy().reshape(n, section)
        out = []
        for j in range(n):
            taken = steps if j == n - 1 else level_steps
            n_hist, level = taken * ALIGN_ROW_WORDS, []
            for p in range(k):
                state = host[j, at_state + p * ALIGN_STATE_WORDS:at_state + (p + 1) * ALIGN_STATE_WORDS]
                hist = host[j, at_hist + p * n_hist:at_hist + (p + 1) * n_hist].reshape(taken, ALIGN_ROW_WORDS)
                level.append((state[:12].view(np.float64).reshape(3, 4).copy(),
                              host[j, at_work + p * 8:at_work + (p + 1) * 8].view(np.float32).reshape(4, 4).copy(),
                              int(state[12]), int(state[13]), hist[:, :4].copy(), hist[:, 4:].copy().view(np.float64),
                              host[j, at_sums + p * INFO_VALUES:at_sums + (p + 1) * INFO_VALUES].copy()))
            out.append(level)
        return out

    def _history(self, hist, xis) -> list:
        """The history's integers [steps,4] and xi [steps,6] in ``PoseAlignment.history``'s format."""
        return [(ALIGN_STATUS[int(r[0])], int(r[1]), int(r[2]), float(r[3]) / INFO_ONE, np.array(x, dtype=np.float64))
                for r, x in zip(hist, xis)]

    # ---- pose alignment: Gauss-Newton steps on those normal equations, iterated on the device (csrc/map_align.hip) ----
    def _align_launch(self, depth: Tensor, intr: Tuple[float, float, float, float], w2c: Tensor, keep: float,
                      beyond: float, kappa: float, near: float, steps: int, damping: float, min_used: int,
                      max_rot: float, max_trans: float, eps_rot: float, eps_trans: float, n_rows: Optional[int] = None,
                      photo=None):
        """w2c [4,4] float32 on the host.  Its copy to the device, the entry point and the read-back of one buffer, the
        call's one synchronisation: (pose [3,4] float64, working pose [4,4] float32, steps applied, rows [steps,4] int64
        = (status, used, tested, rss_fixed), xi [steps,6] float64).  n_rows: the first rows of the map that are summed
        over (None: the live ones).  photo: None, or (intensity, scale, max residual): gsl_map_pose_align_photo."""
        assert depth.is_cuda, "GaussianMap.align_pose: the pose is aligned by HIP kernels, no CPU path"
        lib, st, ptr = _lib.load_library(), _lib.current_stream(), _lib.ptr
        n_state, n_hist = ALIGN_STATE_WORDS, ALIGN_MAX_STEPS * ALIGN_ROW_WORDS
        if self._align is None:
            self._align = dict(words=torch.zeros(n_state + n_hist + 8 + INFO_VALUES, dtype=torch.int64, device=self.device),
                               start=torch.empty(16, device=self.device))
        a = self._align
        n_rows = self.n_live if n_rows is None else int(n_rows)
        words, base = a["words"], a["words"].data_ptr()
        a["start"].copy_(w2c.reshape(16))
        args = (ptr(self.means), n_rows, ptr(a["start"]), *intr, ptr(depth), self.W, self.H, keep, beyond, kappa, near,
                steps, damping, min_used, max_rot, max_trans, eps_rot, eps_trans, base + 8 * (n_state + n_hist + 8),
                base + 8 * (n_state + n_hist), base, base + 8 * n_state)
        if photo is None:
            _lib.check(lib.gsl_map_pose_align(*args, st), "gsl_map_pose_align")
        else:
            _lib.check(lib.gsl_map_pose_align_photo(*args, ptr(self.colors), ptr(photo[0]), photo[1], photo[2], st),
                       "gsl_map_pose_align_photo")
        host = words.cpu().numpy()
        hist = host[n_state:n_state + steps * ALIGN_ROW_WORDS].reshape(steps, ALIGN_ROW_WORDS)
        return (host[:12].view(np.float64).reshape(3, 4).copy(),
                host[n_state + n_hist:n_state + n_hist + 8].view(np.float32).reshape(4, 4).copy(), int(host[12]),
                hist[:, :4].copy(), hist[:, 4:].copy().view(np.float64))

    def _align_params(self, steps, rho, kappa, damping, max_rot_deg, max_trans, eps_rot_deg, eps_trans, min_used):
        """The keyword arguments of ``align_pose`` / ``align_poses`` with their defaults filled in, checked, in the units
        of the entry points: (steps, keep, beyond, kappa, damping, min_used, max_rot [rad], max_trans, eps_rot [rad],
        eps_trans)."""
        cfg = self.cfg
        steps = int(cfg.align_steps if steps is None else steps)
        if not 1 <= steps <= ALIGN_MAX_STEPS:
            raise ValueError(f"steps {steps!r}: a whole number of iterations, 1 .. {ALIGN_MAX_STEPS}")
        if rho is None:
            rho = cfg.depth_rho if cfg.align_rho is None else cfg.align_rho
        if not 0.0 <= rho < 1.0:
            raise ValueError(f"rho {rho!r}: a fraction of the observed depth, inside [0, 1)")
        kappa = float(cfg.info_kappa if kappa is None else kappa)
        if not (math.isfinite(kappa) and kappa >= 0.0):
            raise ValueError(f"kappa {kappa!r}: a fraction of the inverse depth, finite and not negative")
        damping = float(cfg.align_damping if damping is None else damping)
        if not (math.isfinite(damping) and damping >= 0.0):
            raise ValueError(f"damping {damping!r}: an eigenvalue of H / used, finite and not negative")
        max_rot = math.radians(float(cfg.align_max_rot_deg if max_rot_deg is None else max_rot_deg))
        max_trans = float(cfg.align_max_trans if max_trans is None else max_trans)
        eps_rot = math.radians(float(cfg.align_eps_rot_deg if eps_rot_deg is None else eps_rot_deg))
        eps_trans = float(cfg.align_eps_trans if eps_trans is None else eps_trans)
        if not (math.isfinite(max_rot) and max_rot > 0.0 and math.isfinite(max_trans) and max_trans > 0.0):
            raise ValueError(f"max_rot_deg / max_trans {max_rot_deg!r} / {max_trans!r}: finite and above 0")
        if not (math.isfinite(eps_rot) and eps_rot >= 0.0 and math.isfinite(eps_trans) and eps_trans >= 0.0):
            raise ValueError(f"eps_rot_deg / eps_trans {eps_rot_deg!r} / {eps_trans!r}: finite and not negative")
        min_used = int(min_used)
        if min_used < ALIGN_MIN_USED:
            raise ValueError(f"min_used {min_used!r}: at least {ALIGN_MIN_USED} rows")
        keep, beyond = float(np.float32(1.0) - np.float32(rho)), float(np.float32(1.0) + np.float32(rho))
        return (steps, keep, beyond, float(np.float32(kappa)), damping, min_used, max_rot, max_trans, eps_rot, eps_trans)

    @torch.no_grad()
    def align_pose(self, depth, K, c2w, near_plane: float, steps: Optional[int] = None, rho: Optional[float] = None,
                   kappa: Optional[float] = None, damping: Optional[float] = None, max_rot_deg: Optional[float] = None,
                   max_trans: Optional[float] = None, eps_rot_deg: Optional[float] = None,
                   eps_trans: Optional[float] = None, min_used: int = ALIGN_MIN_USED,
                   rows: Optional[int] = None, intensity=None, photo_scale: Optional[float] = None,
                   photo_max_residual: Optional[float] = None, levels: Optional[int] = None,
                   level_steps: Optional[int] = None, pyramid: Optional[FramePyramid] = None) -> PoseAlignment:
        """The pose c2w [4,4] aligned to the map against the depth frame [H,W] (metres): up to ``steps`` (None:
        ``align_steps``) damped Gauss-Newton steps on the normal equations of ``pose_information`` -- the rows chosen
        with ``rho`` (None: ``align_rho``, and ``depth_rho`` when that is None) and ``kappa`` (None: ``info_kappa``),
        ``damping`` (None: ``align_damping``) times the rows used on the diagonal -- each of them solved, bounded
        (``max_rot_deg`` / ``max_trans``), applied and tested for convergence (``eps_rot_deg`` / ``eps_trans``) on the
        device in float64 (the rule: include/gsloc_hip.h).  The start is rounded to float32 as every pose a kernel is
        given.  Changes nothing in the map.  One fixed sequence of 1 + 3 ``steps`` launches, one read-back; an empty
        map gives status FEW without a launch.  The result has to be checked by the caller: a start too far off can
        settle elsewhere (NOTES.md, "Pose alignment").  rows: only the first that many rows of the map are used
        (``loop_constraint``; None: every live row).  intensity, photo_scale, photo_max_residual: as for
        ``pose_information`` -- the normal equations of every iteration then hold the photometric term
        (gsl_map_pose_align_photo: the same launches, the sums of csrc/map_photo.hip).  levels (None:
        ``align_levels``): 0 is all of the above, bit for bit; 1 .. 4 aligns coarse to fine on the frame's image pyramid
        (``pyramid``: a prebuilt one of this frame, or None: built here with ``pyramid_rho``, one more launch) -- the
        pose is aligned at level ``levels`` first, ``level_steps`` iterations (None: ``align_level_steps``, and
        ``steps`` when that is None), then at every level down to the frame itself, ``steps`` iterations there; every
        level is the same entry point with that level's images, size and intrinsics, started on the device at the
        float32 working pose the level before it left (a level that refused left it where it was), and the call keeps
        its one read-back.  The fields of the result are level 0's; ``level_history`` and ``level_steps`` hold every
        level's, coarse to fine."""
        rows = self._prefix(rows)
        photo = self._photo_params(intensity, photo_scale, photo_max_residual)
        (steps, keep, beyond, kappa, damping, min_used, max_rot, max_trans, eps_rot,
         eps_trans) = self._align_params(steps, rho, kappa, damping, max_rot_deg, max_trans, eps_rot_deg, eps_trans, min_used)
        levels, level_steps = self._levels_params(levels, level_steps, steps)
        pyramid_keep = self._pyramid_keep(None, rho) if levels > 0 else None
        depth = self._depth_image(depth)
        intr, c2w = _intr_and_pose(K, c2w)
        w2c = _world_to_camera(c2w)
        if (self.n_live if rows is None else rows) == 0:
            pose, n, hist, xis = w2c.numpy()[:3].astype(np.float64), 0, np.zeros((1, 4), np.int64), np.zeros((1, 6))
            hist[0, 0] = ALIGN_STATUS.index("FEW")
        elif levels > 0:
            frames = self._level_frames(depth, intr, photo, levels, pyramid, pyramid_keep)
            per_level = self._align_levels_launch(frames, w2c.contiguous(), keep, beyond, kappa, float(near_plane), steps,
                                                  level_steps, damping, min_used, max_rot, max_trans, eps_rot, eps_trans,
                                                  n_rows=rows)
            pose, _, n, hist, xis = per_level[-1]
            out = self._alignment(pose, n, hist, xis)
            out.level_history = [self._history(lv[3], lv[4]) for lv in per_level]
            out.level_steps = [int(lv[2]) for lv in per_level]
            return out
        else:
            prefix = {} if rows is None else dict(n_rows=rows)
            if photo is not None:
                prefix["photo"] = photo
            pose, _, n, hist, xis = self._align_launch(depth, intr, w2c.contiguous(), keep, beyond, kappa,
                                                       float(near_plane), steps, damping, min_used, max_rot, max_trans,
                                                       eps_rot, eps_trans, **prefix)
        return self._alignment(pose, n, hist, xis)

    def _alignment(self, pose, n, hist, xis, final: Optional[PoseInformation] = None) -> PoseAlignment:
        """The ``PoseAlignment`` of what a launch read back: the pose [3,4] float64, the steps applied, the history's
        integers [steps,4] and xi [steps,6]; final: the information at the final pose of a closed pose."""
        w2c64 = np.eye(4)
        w2c64[:3] = pose
        history = self._history(hist, xis)
        aligned = torch.from_numpy(np.linalg.inv(w2c64).astype(np.float32)).to(self.device)
        return PoseAlignment(aligned, w2c64, history[-1][0], int(n), history[-1][1], history[-1][2], history,
                             closed=final is not None, final=final)

    # ---- the same for several poses in one call, a finished pose closed by its final sums (csrc/map_align_batch.hip) ---
    def _align_batch_launch(self, depth: Tensor, intr: Tuple[float, float, float, float], w2c: Tensor, keep: float,
                            beyond: float, kappa: float, near: float, steps: int, damping: float, min_used: int,
                            max_rot: float, max_trans: float, eps_rot: float, eps_trans: float,
                            n_rows: Optional[int] = None, photo=None) -> list:
        """w2c [k,4,4] float32 on the host, k <= 16.  Their copy to the device, the entry point and the read-back of one
        buffer, the call's one synchronisation.  Per pose: (pose [3,4] float64, working pose [4,4] float32, steps
        applied, done, rows [steps,4] int64, xi [steps,6] float64, sums [30] int64).  photo: None, or (intensity,
        scale, max residual): gsl_map_pose_align_batch_photo."""
        assert depth.is_cuda, "GaussianMap.align_poses: the poses are aligned by HIP kernels, no CPU path"
        lib, st, ptr = _lib.load_library(), _lib.current_stream(), _lib.ptr
        cap, k = ALIGN_BATCH_MAX_POSES, int(w2c.shape[0])
        n_hist = steps * ALIGN_ROW_WORDS  # the history is laid out for this call's steps
        at_state, at_hist = 0, cap * ALIGN_STATE_WORDS  # offsets in 8-byte words; the sections are sized for 16 poses
        at_work = at_hist + cap * ALIGN_MAX_STEPS * ALIGN_ROW_WORDS
        at_sums = at_work + cap * 8
        if self._align_batch is None:
            self._align_batch = dict(words=torch.zeros(at_sums + cap * INFO_VALUES, dtype=torch.int64, device=self.device),
                                     start=torch.empty(cap, 16, device=self.device))
        a = self._align_batch
        n_rows = self.n_live if n_rows is None else int(n_rows)
        words, base = a["words"], a["words"].data_ptr()
        a["start"][:k].copy_(w2c.reshape(k, 16))
        args = (ptr(self.means), n_rows, ptr(a["start"]), k, *intr, ptr(depth), self.W, self.H, keep, beyond, kappa, near,
                steps, damping, min_used, max_rot, max_trans, eps_rot, eps_trans, base + 8 * at_sums, base + 8 * at_work,
                base + 8 * at_state, base + 8 * at_hist)
        if photo is None:
            _lib.check(lib.gsl_map_pose_align_batch(*args, st), "gsl_map_pose_align_batch")
        else:
            _lib.check(lib.gsl_map_pose_align_batch_photo(*args, ptr(self.colors), ptr(photo[0]), photo[1], photo[2], st),
                       "gsl_map_pose_align_batch_photo")
        host = words.cpu().numpy()
        out = []
        for p in range(k):
            state = host[at_state + p * ALIGN_STATE_WORDS:at_state + (p + 1) * ALIGN_STATE_WORDS]
            hist = host[at_hist + p * n_hist:at_hist + (p + 1) * n_hist].reshape(steps, ALIGN_ROW_WORDS)
            out.append((state[:12].view(np.float64).reshape(3, 4).copy(),
                        host[at_work + p * 8:at_work + (p + 1) * 8].view(np.float32).reshape(4, 4).copy(),
                        int(state[12]), int(state[13]), hist[:, :4].copy(), hist[:, 4:].copy().view(np.float64),
                        host[at_sums + p * INFO_VALUES:at_sums + (p + 1) * INFO_VALUES].copy()))
        return out

    @torch.no_grad()
    def align_poses(self, depth, K, c2ws, near_plane: float, steps: Optional[int] = None, rho: Optional[float] = None,
                    kappa: Optional[float] = None, damping: Optional[float] = None, max_rot_deg: Optional[float] = None,
                    max_trans: Optional[float] = None, eps_rot_deg: Optional[float] = None,
                    eps_trans: Optional[float] = None, min_used: int = ALIGN_MIN_USED,
                    rows: Optional[int] = None, intensity=None, photo_scale: Optional[float] = None,
                    photo_max_residual: Optional[float] = None, levels: Optional[int] = None,
                    level_steps: Optional[int] = None, pyramid: Optional[FramePyramid] = None) -> list:
        """``align_pose`` for each of the poses c2ws [k,4,4] (a tensor, or a sequence of [4,4] poses) against the same
        frame, with the same keyword arguments and defaults: one call of 1 + 3 ``steps`` launches and one read-back for
        up to 16 poses (more go in chunks of 16).  Pose, status, steps and history of every ``PoseAlignment`` are bit
        for bit ``align_pose``'s.  On the device a pose that has finished stops paying for its sums, after one more
        pass at its final pose: the result is then ``closed`` and ``final`` holds those sums as a ``PoseInformation``
        (with ``info_min_eig``) -- what ``pose_information`` gives at c2w, without another launch.  A pose that
        converges on the last iteration is not closed.  An empty map gives status FEW, not closed, without a launch.
        intensity, photo_scale, photo_max_residual: as for ``align_pose`` (gsl_map_pose_align_batch_photo); ``final``
        then holds geometry plus colour, without the photometric counts (``photo_used`` stays 0).  levels,
        level_steps, pyramid: as for ``align_pose``, every level one batched call for all the poses (the pyramid is the
        frame's: built once); ``closed`` and ``final`` are level 0's."""
        rows = self._prefix(rows)
        photo = self._photo_params(intensity, photo_scale, photo_max_residual)
        (steps, keep, beyond, kappa, damping, min_used, max_rot, max_trans, eps_rot,
         eps_trans) = self._align_params(steps, rho, kappa, damping, max_rot_deg, max_trans, eps_rot_deg, eps_trans, min_used)
        levels, level_steps = self._levels_params(levels, level_steps, steps)
        pyramid_keep = self._pyramid_keep(None, rho) if levels > 0 else None
        poses = [torch.as_tensor(c) for c in c2ws]
        for c in poses:
            if c.shape != (4, 4):
                raise ValueError(f"a pose is {tuple(c.shape)}, not (4, 4)")
        if not poses:
            return []
        depth = self._depth_image(depth)
        intr, _ = _intr_and_pose(K, poses[0])
        w2c = _world_to_camera(torch.stack([c.detach().cpu().double() for c in poses]))
        if (self.n_live if rows is None else rows) == 0:
            hist = np.zeros((1, 4), np.int64)
            hist[0, 0] = ALIGN_STATUS.index("FEW")
            return [self._alignment(w.numpy()[:3].astype(np.float64), 0, hist, np.zeros((1, 6))) for w in w2c]
        min_eig = INFO_MIN_EIG if self.cfg.info_min_eig is None else float(self.cfg.info_min_eig)
        prefix = {} if rows is None else dict(n_rows=rows)
        if photo is not None:
            prefix["photo"] = photo
        out = []
        frames = None if levels == 0 else self._level_frames(depth, intr, photo, levels, pyramid, pyramid_keep)
        for at in range(0, len(poses), ALIGN_BATCH_MAX_POSES):
            chunk = w2c[at:at + ALIGN_BATCH_MAX_POSES].contiguous()
            if frames is not None:
                per_level = self._align_batch_levels_launch(frames, chunk, keep, beyond, kappa, float(near_plane), steps,
                                                            level_steps, damping, min_used, max_rot, max_trans, eps_rot,
                                                            eps_trans, n_rows=rows)
                for p, (pose, _, n, done, hist, xis, sums) in enumerate(per_level[-1]):
                    al = self._alignment(pose, n, hist, xis, information_from_sums(sums, min_eig) if done == 2 else None)
                    al.level_history = [self._history(lv[p][4], lv[p][5]) for lv in per_level]
                    al.level_steps = [int(lv[p][2]) for lv in per_level]
                    out.append(al)
                continue
            for pose, _, n, done, hist, xis, sums in self._align_batch_launch(
                    depth, intr, chunk, keep, beyond, kappa, float(near_plane), steps, damping, min_used, max_rot,
                    max_trans, eps_rot, eps_trans, **prefix):
                out.append(self._alignment(pose, n, hist, xis, information_from_sums(sums, min_eig) if done == 2 else None))
        return out

    # ---- trajectory correction: the rows follow the frame they came from (csrc/map_correct.hip) ----------------------
    @torch.no_grad()
    def rows_up_to(self, frame: int) -> int:
        """How many live rows have an origin <= frame.  The origins are non-decreasing in map order, so these rows are
        the first that many of the map: one ``torch.searchsorted`` and one read-back."""
        if self.origins is None:
            raise RuntimeError("rows_up_to: MapConfig.origins is False, the map keeps no origins")
        if self.n_live == 0:
            return 0
        frame = max(min(int(frame), 2 ** 31 - 1), -1)
        key = torch.tensor([frame], dtype=torch.int32, device=self.origins.device)
        return int(torch.searchsorted(self.origins[: self.n_live], key, right=True).item())

    def _correct_launch(self, table: Tensor) -> Tuple[int, int]:
        """table [n_frames,12] float32 on the host.  Its copy to the device, the entry point (which zeroes the counters)
        over the live rows, in place, and the read-back of (rows moved, rows with an origin outside the table), the
        call's one synchronisation."""
        assert self.means.is_cuda, "GaussianMap.correct: the rows are moved by a HIP kernel, no CPU path"
        lib, st, ptr = _lib.load_library(), _lib.current_stream(), _lib.ptr
        if self._correct_counters is None:
            self._correct_counters = torch.zeros(2, dtype=torch.int64, device=self.device)
        on_device = table.to(self.device).contiguous()
        _lib.check(lib.gsl_map_correct(ptr(self.means), ptr(self.origins), self.n_live, ptr(on_device),
                                       int(table.shape[0]), ptr(self._correct_counters), st), "gsl_map_correct")
        moved, outside = self._correct_counters.tolist()
        return moved, outside

    @torch.no_grad()
    def correct(self, transforms) -> Tuple[int, int]:
        """Moves the live rows with their frames: transforms [n_frames,4,4], per frame of the trajectory the rigid
        transform of the world that takes its old pose to its corrected one (c2w_new = D c2w_old); a row with the
        origin k becomes D_k applied to it, in float32 (the rule: include/gsloc_hip.h).  A row whose D_k is exactly
        the identity, a row that is not finite and a row whose origin lies outside the transforms keeps every bit.
        Only the means move: colours, stamps, weights and origins stay.  In place: ``points`` stays valid and shows the
        moved rows.  The pose of every keyframe with a recorded frame index (``add_keyframe``'s origin) inside the
        transforms moves as well, pose <- D_k pose in float64, stored as float32.  Returns (rows moved, rows with an
        origin outside the transforms).  One copy of the float32 [n_frames,12] table to the device, one zeroing launch,
        one kernel, one read-back; an empty map gives (0, 0) without a launch.  When a row moved, the next
        ``view_violations`` needs a fresh ``select_view``, as after a removal."""
        if self.origins is None:
            raise RuntimeError("correct: MapConfig.origins is False, the map keeps no origins")
        T = torch.as_tensor(transforms).detach().cpu().double().numpy()
        if T.ndim != 3 or T.shape[0] < 1 or T.shape[1:] != (4, 4):
            raise ValueError(f"transforms are {T.shape}, not (n_frames >= 1, 4, 4)")
        if not np.isfinite(T).all():
            raise ValueError("transforms: some entry is not finite")
        moved, outside = 0, 0
        if self.n_live > 0:
            table = np.ascontiguousarray(T[:, :3, :].astype(np.float32).reshape(-1, 12))
            moved, outside = self._correct_launch(torch.from_numpy(table))
        if moved > 0:
            self._view_rows = -1  # the view ballots describe rows that lay elsewhere
        for slot in range(self.n_keyframes):
            k = int(self._kf_origins[slot])
            if 0 <= k < len(T):
                self._kf_poses[slot] = (T[k] @ self._kf_poses[slot].astype(np.float64)).astype(np.float32)
        return int(moved), int(outside)

    @torch.no_grad()
    def loop_constraint(self, depth, K, c2w, upto_frame: int, near_plane: float, **align) -> "LoopConstraint":
        """A loop constraint from the map itself: the pose c2w [4,4] of a frame that sees an old part of the map again,
        aligned against the rows of the frames up to ``upto_frame`` only -- ``rows_up_to(upto_frame)``, a prefix of the
        map; the rows the drifted frames since then wrote beside it take no part -- by ``align_pose`` (``align``: its
        keyword arguments), and the scores (``score_poses``) of the given and of the aligned pose against the same
        prefix.  Changes nothing in the map.  Whether to trust the result, and what to do with it
        (``spread_correction``, ``correct``), is the caller's decision.  ``intensity``, ``photo_scale`` and
        ``photo_max_residual`` among ``align`` go to ``align_pose``: a constraint measured on a textured wall is then
        closed in the wall's plane as well; ``levels``, ``level_steps`` and ``pyramid`` go there too (coarse to fine, a
        constraint at a drifted estimate has the wider basin).  The scores stay depth only."""
        n = self.rows_up_to(upto_frame)
        al = self.align_pose(depth, K, c2w, near_plane, rows=n, **align)
        scores = self.score_poses(depth, K, [torch.as_tensor(c2w).detach().cpu(), al.c2w.detach().cpu()], near_plane,
                                  rows=n)
        return LoopConstraint(al, n, scores[0], scores[1])

    # ---- covisibility: the pose scores' verdicts, binned by the frame a row came from (csrc/map_covis.hip) -----------
    def _covis_launch(self, depth: Tensor, intr: Tuple[float, float, float, float], w2c: Tensor, near: float,
                      n_frames: int, n_rows: Optional[int] = None) -> Tuple[np.ndarray, int]:
        """w2c [4,4] float32 on the host.  Its copy to the device, the entry point (which zeroes the counts and the
        count of rows outside) and the read-back of one buffer, the call's one synchronisation: (int64 [n_frames,3],
        rows whose origin lies outside the table).  n_rows: the first rows of the map that are judged (None: the live
        ones)."""
        n_rows = self.n_live if n_rows is None else int(n_rows)
        assert depth.is_cuda, "GaussianMap.covisibility: the rows are judged and counted by a HIP kernel, no CPU path"
        lib, st, ptr = _lib.load_library(), _lib.current_stream(), _lib.ptr
        if self._covis is None or self._covis["words"].numel() < 2 + 3 * n_frames:
            # one buffer of 4-byte words: [the rows outside, one 64-bit word][counts, 3 per frame]
            self._covis = dict(words=torch.empty(2 + 3 * max(n_frames, 64), dtype=torch.int32, device=self.device),
                               pose=torch.empty(16, device=self.device))
        c = self._covis
        c["pose"].copy_(w2c.reshape(16))
        base = c["words"].data_ptr()
        _lib.check(lib.gsl_map_covis(ptr(self.means), ptr(self.origins), n_rows, ptr(c["pose"]), *intr, ptr(depth),
                                     self.W, self.H, self.keep, self.beyond, near, n_frames, base + 8, base, st),
                   "gsl_map_covis")
        host = c["words"][: 2 + 3 * n_frames].cpu().numpy()
        return host[2:].astype(np.int64).reshape(n_frames, 3), int(host[:2].copy().view(np.int64)[0])

    @torch.no_grad()
    def covisibility(self, depth, K, c2w, near_plane: float, n_frames: Optional[int] = None,
                     rows: Optional[int] = None) -> np.ndarray:
        """Which frames' rows the depth frame [H,W] (metres) sees from the pose c2w [4,4], and whether they agree with
        it: int64 [n_frames,3], per frame of the trajectory the rows it appended (``origins``) that the frame TESTS,
        those that AGREE and those in FRONT -- the verdicts of ``score_poses`` for that one pose, with the map's own
        ``keep`` and ``beyond``, binned by origin, so that the sum over the frames is ``score_poses(depth, K, [c2w],
        near_plane)[0]`` whenever no origin lies outside.  n_frames: the frames of the table (None: the last origin
        written + 1); a row with an origin outside it is counted in ``last_covis_outside`` and nowhere else.  rows:
        only the first that many rows of the map are judged (None: every live row).  Changes nothing in the map.  Two
        zeroing launches, one kernel, one read-back; an empty map gives zeros without a launch."""
        if self.origins is None:
            raise RuntimeError("covisibility: MapConfig.origins is False, the map keeps no origins")
        rows = self._prefix(rows)
        if n_frames is None:
            n_frames = max(self._last_origin + 1, 1)
        if isinstance(n_frames, bool) or not isinstance(n_frames, (int, np.integer)) or not 1 <= n_frames <= 2 ** 24:
            raise ValueError(f"n_frames {n_frames!r}: a whole number of frames, 1 .. 2^24")
        n_frames = int(n_frames)
        depth = self._depth_image(depth)
        intr, c2w = _intr_and_pose(K, c2w)
        self.last_covis_outside = 0
        if (self.n_live if rows is None else rows) == 0:
            return np.zeros((n_frames, 3), dtype=np.int64)
        prefix = {} if rows is None else dict(n_rows=rows)
        counts, self.last_covis_outside = self._covis_launch(depth, intr, _world_to_camera(c2w).contiguous(),
                                                             float(near_plane), n_frames, **prefix)
        return counts

    # ---- refinement: the rows a depth frame observes again move to the running mean of their depths (csrc/map_refine.hip)
    def _refine_launch(self, depth: Tensor, rgb: Optional[Tensor], intr: Tuple[float, float, float, float], w2c: Tensor,
                       cam: Tuple[float, float, float], near: float) -> int:
        """The entry point (which zeroes the counter) over the live rows, in place, and the read-back of the rows
        refined, the call's one synchronisation."""
        assert depth.is_cuda, "GaussianMap.refine: the rows are refined by a HIP kernel, no CPU path"
        lib, st, ptr = _lib.load_library(), _lib.current_stream(), _lib.ptr
        _lib.check(lib.gsl_map_refine(ptr(self.means), None if rgb is None else ptr(self.colors), ptr(self.weights),
                                      self.n_live, ptr(w2c), *cam, *intr, ptr(depth), ptr(rgb), self.W, self.H,
                                      self._refine_keep, near, int(self.cfg.refine_max_weight),
                                      ptr(self._refine_counter), st), "gsl_map_refine")
        return self._refine_counter.tolist()[0]

    @torch.no_grad()
    def refine(self, depth, rgb, K, c2w, near: float) -> int:
        """Moves the live rows that the depth frame [H,W] (metres) at the pose c2w [4,4] observes again -- they project
        into the image beyond ``near`` and each of the four pixels around their projection shows their depth within
        ``refine_rho`` either way -- along their own ray to the running mean of the depths observed there, and raises
        their weight by one up to ``refine_max_weight`` (the rule: include/gsloc_hip.h); every other row keeps every
        bit.  rgb [H,W,3] in 0..255: their colours go to the running mean of the image at their projection as well;
        None: the colours are left alone.  In place: ``points`` / ``point_colors`` stay valid and show the refined
        rows.  Returns the rows refined.  One zeroing launch, one kernel, one read-back; an empty map gives 0 without
        a launch."""
        if self.weights is None:
            raise RuntimeError("refine: MapConfig.refine is False, the map keeps no weights")
        if self.n_live == 0:
            return 0
        depth = self._depth_image(depth)
        if rgb is not None:
            rgb = self._image(torch.as_tensor(rgb)[..., :3], (self.H, self.W, 3), "rgb")
        intr, c2w = _intr_and_pose(K, c2w)
        w2c = _world_to_camera(c2w).to(self.device).contiguous()
        cam = tuple(float(t) for t in c2w.detach().cpu()[:3, 3].to(torch.float32))
        return self._refine_launch(depth, rgb, intr, w2c, cam, float(near))

    # ---- place recognition: keyframes, their depth descriptors and the match of a frame against them (csrc/map_place.hip)
    def _place_buffers(self):
        if self._place is None:
            dev, i32 = self.device, torch.int32
            self._place = dict(table=torch.full((int(self.cfg.keyframe_max), PLACE_CELLS), -1, dtype=i32, device=dev),
                               query=torch.full((PLACE_CELLS,), -1, dtype=i32, device=dev),
                               out=torch.zeros(PLACE_MAX_KEYFRAMES, len(PLACE_SHIFTS), 2, dtype=i32, device=dev))
        return self._place

    def _describe_launch(self, depth: Tensor, desc: Tensor) -> None:
        """The descriptor of depth [H,W] into desc, 192 contiguous int32 on the device.  No read-back."""
        assert depth.is_cuda, "GaussianMap.describe: the descriptor is made by a HIP kernel, no CPU path"
        _lib.check(_lib.load_library().gsl_map_place_describe(_lib.ptr(depth), self.W, self.H, _lib.ptr(desc),
                                                              _lib.current_stream()), "gsl_map_place_describe")

    def _match_launch(self, query: Tensor, table: Tensor, n: int) -> np.ndarray:
        """query [192] against the first n rows of table [keyframe_max,192]; the read-back of int64 [n,15,2]: per
        keyframe and shift (common, sum)."""
        assert query.is_cuda, "GaussianMap.match_place: the descriptors are compared by a HIP kernel, no CPU path"
        out = self._place_buffers()["out"]
        _lib.check(_lib.load_library().gsl_map_place_match(_lib.ptr(query), _lib.ptr(table), n, _lib.ptr(out),
                                                           _lib.current_stream()), "gsl_map_place_match")
        return out[:n].cpu().numpy().astype(np.int64)  # the call's one synchronisation

    @property
    def n_keyframes(self) -> int:
        return min(self._kf_made, int(self.cfg.keyframe_max))

    @property
    def keyframe_poses(self) -> Tensor:
        """float32 [n_keyframes,4,4] on the host: the pose of the keyframe in every slot."""
        return torch.from_numpy(self._kf_poses[: self.n_keyframes].copy())

    @torch.no_grad()
    def describe(self, depth) -> Tensor:
        """int32 [192] on the device: the 16 x 12 descriptor of the depth frame [H,W] (metres) -- per cell of the image
        the mean of the valid depths in units of 1 / 1024 m, or -1 where fewer than half of the cell's pixels have one
        (the rule: include/gsloc_hip.h).  One launch, no read-back."""
        depth = self._depth_image(depth)
        desc = torch.empty(PLACE_CELLS, dtype=torch.int32, device=self.device)
        self._describe_launch(depth, desc)
        return desc

    @torch.no_grad()
    def add_keyframe(self, depth, c2w, origin: Optional[int] = None) -> Optional[int]:
        """Keeps the frame -- its pose c2w [4,4] on the host, its descriptor on the device -- as a keyframe when the
        pose is further than ``keyframe_rot_deg`` degrees or further than ``keyframe_trans`` metres from the pose of
        every stored keyframe (the first frame always is one); decided on the host from the stored poses alone, and
        only then is the descriptor launched, straight into the keyframe's row of the device table.  Returns the slot,
        or None.  With ``keyframe_max`` keyframes stored the oldest one is overwritten (a ring).  No read-back.

        Keyframes describe frames, not rows: eviction, free space and merging leave them alone.  A keyframe whose rows
        have all gone is harmless -- the candidate poses around it test too few rows and are rejected by the rule that
        every estimate is held against (``reloc_min_tested``).

        origin: the index of the frame in the caller's trajectory; ``correct`` moves the pose of a keyframe that has
        one with its frame, and leaves a keyframe without one (None) alone."""
        if origin is not None and (isinstance(origin, bool) or not isinstance(origin, (int, np.integer)) or origin < 0):
            raise ValueError(f"origin {origin!r}: a whole frame index, at least 0 (or None)")
        if not self.cfg.keyframes:
            raise RuntimeError("add_keyframe: MapConfig.keyframes is False, the map keeps no keyframes")
        depth = self._depth_image(depth)
        pose = torch.as_tensor(c2w)
        if pose.shape != (4, 4):
            raise ValueError(f"c2w is {tuple(pose.shape)}, not (4, 4)")
        pose = pose.detach().cpu().to(torch.float32).numpy()
        n = self.n_keyframes
        if n > 0:
            stored, new = self._kf_poses[:n].astype(np.float64), pose.astype(np.float64)
            dist = np.linalg.norm(stored[:, :3, 3] - new[None, :3, 3], axis=1)
            # the angle of R_stored^T R_new, from its trace
            cos = (np.einsum("kij,ij->k", stored[:, :3, :3], new[:3, :3]) - 1.0) / 2.0
            angle = np.degrees(np.arccos(np.clip(cos, -1.0, 1.0)))
            far = (angle > float(self.cfg.keyframe_rot_deg)) | (dist > float(self.cfg.keyframe_trans))
            if not bool(far.all()):
                return None
        slot = self._kf_made % int(self.cfg.keyframe_max)
        self._describe_launch(depth, self._place_buffers()["table"][slot])
        self._kf_poses[slot] = pose
        self._kf_origins[slot] = -1 if origin is None else int(origin)
        self._kf_made += 1
        return slot

    @torch.no_grad()
    def match_place(self, depth) -> list:
        """The stored keyframes that the depth frame [H,W] resembles, the most similar first: a list of
        (slot, sx, sy, sum, common).  One descriptor launch, one match launch of the frame's descriptor against all
        keyframes under the 15 shifts sx in -2 .. 2, sy in -1 .. 1 of the grid (the rule: include/gsloc_hip.h) and one
        read-back; then, in Python integers, every keyframe's shift with the smallest sum / common among those with
        ``common >= place_min_common``, and the keyframes in ascending order of that value.  Fractions are compared
        exactly (cross-multiplied); ties go to the smaller |sx| + |sy|, then the earlier shift, then the lower slot.
        Keyframes with no admissible shift are left out; no keyframes: an empty list without a launch."""
        if not self.cfg.keyframes:
            raise RuntimeError("match_place: MapConfig.keyframes is False, the map keeps no keyframes")
        n = self.n_keyframes
        if n == 0:
            return []
        depth, p = self._depth_image(depth), self._place_buffers()
        self._describe_launch(depth, p["query"])
        result = self._match_launch(p["query"], p["table"], n)
        return rank_places(result, int(self.cfg.place_min_common))


def rank_places(result, min_common: int) -> list:
    """``GaussianMap.match_place``'s ranking of [n,15,2] (common, sum) pairs: [(slot, sx, sy, sum, common), ...]."""

    def better(a, b) -> bool:
        """a, b: (sum, common, |sx| + |sy|, shift, slot).  sum_a / common_a < sum_b / common_b, exactly; then the
        rest in order."""
        left, right = a[0] * b[1], b[0] * a[1]
        return left < right or (left == right and a[2:] < b[2:])

    best = []
    for slot, per_shift in enumerate(np.asarray(result).tolist()):
        top = None
        for s, (common, total) in enumerate(per_shift):
            if common < max(int(min_common), 1):
                continue
            sx, sy = PLACE_SHIFTS[s]
            entry = (int(total), int(common), abs(sx) + abs(sy), s, slot)
            if top is None or better(entry, top):
                top = entry
        if top is not None:
            best.append(top)
    ranked = sorted(best, key=functools.cmp_to_key(lambda a, b: -1 if better(a, b) else int(better(b, a))))
    return [(slot, PLACE_SHIFTS[s][0], PLACE_SHIFTS[s][1], total, common) for total, common, _, s, slot in ranked]
