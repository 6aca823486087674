"""GPU: Localizer(mode="map") with MapConfig.align_accept and MapConfig.reloc_align_top on real kernels, at 160x120.

(a) The constant twist of tests/test_gpu_map_align_localizer.py (6 frames, 0.4 degrees and 1 cm a frame, the real
    tracker), once with align=True and once with align_accept=True added.  On the numpy mirror every one of the five
    alignments of this sequence converges at its third iteration of eight, is closed, uses 16 700 .. 17 600 rows and has
    a smallest eigenvalue of H / used of 0.034 .. 0.036 (INFO_MIN_EIG is 1e-3): at least 4 of the 5 frames must be
    direct.  A direct frame reports no step.  The direct run's ATE (the RMS of the translation errors over all six
    poses) may exceed the tracked run's by 1.5e-4 m at the most: one step of the depth files, 1 / 6553.5 m, the bias
    NOTES.md names for the aligned start.  Both are printed.
(b) One wall: constant-depth frames, the camera backing away from a wall by 1 cm a frame, and tests/test_map_cpu._Tracker
    as the tracker (it answers the pose it is given as ground truth), as in tests/test_gpu_map_loop.py.  The alignment
    converges along the wall's normal and three directions stay open: no frame is direct, direct_reason is "weak", and
    poses, steps and the map's rows are bit for bit those of the run with align=True alone.
(c) The lost frame of tests/test_gpu_map_reloc_localizer.py (b) -- real scoring, a stand-in tracker that answers its
    start -- moved off the grid by 2.2 cm and half a degree, so that no candidate is the frame's pose.  With
    reloc_align_top=4 at least one candidate is replaced by its alignment, the frame is relocalised, and the start that
    is chosen is no further from the ground truth than the start chosen with the option at 0.  Both distances are
    printed.

Measured on the MI355X: the docstrings of the tests."""
import math

import numpy as np
import pytest
import torch

from gsplatloc_amd.localizer import Localizer, reloc_candidates
from gsplatloc_amd.mapping import MapConfig
from gsplatloc_amd.my_gsplat import TrackerConfig
from gsplatloc_amd.synthetic import replica_intrinsics, room_depth
from tests import test_map_cpu as base
from tests.pose_ref import axis_angle
from tests.test_gpu_map_align_localizer import _run
from tests.test_gpu_map_localizer import H, ITERS, N_B, W, seq_b  # noqa: F401
from tests.test_gpu_map_reloc_localizer import STEP_B, YAW_B, _StartTracker

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _ate(run):
    err = (run["traj"][:, :3, 3] - run["gts"][:, :3, 3].to(run["traj"].device)).norm(dim=1)
    return math.sqrt(float((err * err).mean()))


def test_direct_frames_on_the_constant_twist(seq_b, capsys):  # noqa: F811
    """MI355X: 5 of 5 frames direct, each 7.65e-5 .. 7.68e-5 m from the truth (tracked: 3.6e-4 .. 7.0e-4 m after 302 .. 693
    steps); ATE 7.00e-5 m direct against 4.68e-4 m tracked."""
    tracked = _run(seq_b, MapConfig(align=True))
    direct = _run(seq_b, MapConfig(align=True, align_accept=True))
    ate_t, ate_d = _ate(tracked), _ate(direct)
    res = direct["results"]
    with capsys.disabled():
        print(f"[align direct] (a) direct {[r.direct for r in res]}, reasons {[r.direct_reason for r in res]}, steps "
              f"{[r.steps for r in res]} against {[r.steps for r in tracked['results']]} tracked; eT per frame "
              f"{['%.3e' % r.eT for r in res]} against {['%.3e' % r.eT for r in tracked['results']]}; ATE direct "
              f"{ate_d:.3e} m, tracked {ate_t:.3e} m")
    assert all(r.direct is None and r.direct_reason is None for r in tracked["results"])
    assert sum(bool(r.direct) for r in res) >= 4 and len(res) == N_B - 1 == 5
    for r in res:
        assert not r.lost and r.added >= 0
        if r.direct:
            assert (r.steps, r.best_step, r.best_loss, r.direct_reason) == (0, -1, None, None)
            assert r.aligned is True and r.align_status == "CONVERGED" and torch.equal(r.c2w, r.init_c2w)
        else:
            assert r.direct_reason in ("status", "open", "share", "used", "weak") and r.steps > 0
    assert direct["loc"].map.n_live == W * H + sum(r.added for r in res)
    assert ate_d <= ate_t + 1.5e-4, (ate_d, ate_t)


def test_one_wall_is_never_direct_and_changes_nothing(capsys):
    """MI355X: every alignment CONVERGED after 2 steps, every frame "weak"; the same bits as with align=True alone."""
    K = replica_intrinsics(W, H)
    depths = [torch.full((H, W), 2.0 + 0.01 * k) for k in range(5)]
    poses = [torch.eye(4) for _ in range(5)]
    for k, p in enumerate(poses):
        p[2, 3] = -0.01 * k  # back along the optical axis: the wall at z = 2 is 2 + 0.01 k away

    def run(**cfg):
        base._Tracker.made = []
        loc = Localizer(K, W, H, TrackerConfig(max_steps=5), normalize=False, motion="hold", device=DEV,
                        tracker_factory=base._Tracker, mode="map", map_config=MapConfig(align=True, **cfg))
        loc.reset(depths[0], None, poses[0])
        return loc, [loc.track(depths[k], None, gt_c2w=poses[k]) for k in range(1, 5)]

    plain, want = run()
    loc, got = run(align_accept=True)
    with capsys.disabled():
        print(f"[align direct] (b) one wall: {[(r.align_status, r.align_steps, r.direct_reason) for r in got]}, aligned "
              f"{[r.aligned for r in got]}")
    assert all(r.direct is False and r.direct_reason == "weak" for r in got)
    assert all(r.direct is None for r in want)
    for a, b in zip(got, want):
        assert torch.equal(a.c2w, b.c2w) and torch.equal(a.init_c2w, b.init_c2w)
        assert (a.steps, a.best_step, a.best_loss, a.added, a.map_size, a.lost, a.aligned, a.align_status, a.align_steps) == (
            b.steps, b.best_step, b.best_loss, b.added, b.map_size, b.lost, b.aligned, b.align_status, b.align_steps)
    assert torch.equal(loc.trajectory, plain.trajectory)
    assert loc.map.n_live == plain.map.n_live and torch.equal(loc.map.points, plain.map.points)
    assert torch.equal(loc.map.point_colors, plain.map.point_colors)


def test_aligned_candidates_relocalise_a_frame_off_the_grid(capsys):
    """MI355X: 3 of 4 candidates replaced; the chosen start 7.5e-7 m from the truth against 2.24e-2 m with the option
    at 0."""
    K = replica_intrinsics(W, H)
    pose0 = torch.eye(4)
    pose0[:3, :3] = axis_angle((0.0, 1.0, 0.0), YAW_B).float()
    cands = reloc_candidates([pose0], MapConfig().reloc_rot_deg, STEP_B, MapConfig().reloc_levels)
    off = torch.eye(4)
    off[:3, :3] = axis_angle((0.0, 1.0, 0.0), 0.5).float()
    off[0, 3], off[2, 3] = 0.02, -0.01
    pose1 = cands[1 + 6 * MapConfig().reloc_levels] @ off  # one grid step along x, and a little more
    gen = torch.Generator().manual_seed(5)
    frames = [(room_depth(W, H, K, p), torch.randint(0, 255, (H, W, 3), generator=gen).float()) for p in (pose0, pose1)]
    out = {}
    for top in (0, 4):
        _StartTracker.made = []
        loc = Localizer(K, W, H, TrackerConfig(max_steps=ITERS), normalize=False, motion="hold",
                        tracker_factory=_StartTracker, mode="map",
                        map_config=MapConfig(reloc=True, reloc_trans=STEP_B, reloc_align_top=top))
        loc.reset(*frames[0], pose0)
        r = loc.track(*frames[1], gt_c2w=pose1)
        starts = [s for t in _StartTracker.made for s in t.starts]
        assert len(starts) == 2 and torch.equal(starts[0].cpu(), pose0) and torch.equal(starts[1], r.init_c2w)
        out[top] = (r, float((r.init_c2w[:3, 3].cpu() - pose1[:3, 3]).norm()))
    (r0, d0), (r4, d4) = out[0], out[4]
    with capsys.disabled():
        print(f"[align direct] (c) reloc_align_top 4: {r4.reloc_aligned} of 4 candidates replaced, relocalised "
              f"{r4.relocalised}, (tested, agree, front) {(r4.tested, r4.agree, r4.front)}; the chosen start is {d4:.3e} m "
              f"from the truth, {d0:.3e} m with the option at 0 ((tested, agree, front) {(r0.tested, r0.agree, r0.front)})")
    assert r0.reloc_aligned is None and r0.relocalised is True and 0.02 < d0 < 0.03  # the grid's nearest candidate
    assert r4.reloc_aligned >= 1 and (r4.relocalised, r4.lost) == (True, False)
    assert d4 <= d0
    assert r4.direct is None and r4.steps == 24 and r4.added > 0
    assert np.isfinite(r4.eT) and r4.eT == pytest.approx(d4, abs=1e-6)  # the stand-in tracker answers its start
