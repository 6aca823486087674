"""GPU: Localizer(mode="map") with MapConfig.view_guard_px -- every frame tracked against the rows of the map that are in
view from its start pose -- at 160x120, "ED", with the settings and the yardstick of tests/test_gpu_map_localizer.py.

(a) Neutral when everything is in view: the 6-frame constant twist of that file with a guard of 10 image widths.  The
    uncut map mode is run twice in this process first.  If the two uncut runs repeat bit for bit (poses, step counts,
    added rows), the culled run must equal them bit for bit; if they do not, it must lie within their difference
    (largest absolute pose entry, step count and added rows per frame).  Measured on the MI355X: they repeat bit for
    bit -- difference 0 in every pose entry, steps 349, 648, 321, 572, 356 and added rows 120, 120, 145, 135, 130 both
    times -- and the culled run gave the same bits.
(b) A sweep that outgrows the view: the camera turns by 1 degree about (0.3, 1, -0.2) and moves 1 cm every frame, 16
    frames (15 steps), guard 8 px.  With the ground-truth poses and frame 0's points the rule leaves 23.0 % of them out
    at the last pose (asserted here with the mirror: at least 20 %).  No frame is lost; the per-frame absolute error
    stays under the bound of the map test, twice the running sum of the ground-truth-start yardstick's pair errors on this sequence;
    `tracked` is the mirror's count at every frame's start pose and falls below the map's rows from the frame where the
    mirror first leaves a row out; the rows added in total are at most 1.5 x those of the uncut run (a band that fails
    unchecked re-inserts the strip that leaves the view -- as wide as the one that enters: twice the additions).
(c) The check bites: the same sweep with view_guard_px = view_reach_px, the smallest legal guard.  view_violations > 0 on
    at least one frame, and the bound on the added rows still holds."""
import numpy as np
import pytest
import torch

from gsplatloc_amd.mapping import MapConfig
from gsplatloc_amd.synthetic import write_replica_constant_twist
from tests import map_view_ref as ref
from tests.test_gpu_map_localizer import ITERS, N_B, H, W, _check_drift, _check_growth, _yardstick

pytestmark = pytest.mark.gpu
N_SWEEP, SWEEP_DEG, SWEEP_TRANS, GUARD = 16, 1.0, 0.01, 8.0


def _run(root, n_frames, map_config):
    """Localizer(mode="map") over the sequence; besides what tests/test_gpu_map_localizer.py's _run returns, the live
    rows before every frame (host copies), for the mirror."""
    from gsplatloc_amd.data import Parser
    from gsplatloc_amd.localizer import Localizer
    from gsplatloc_amd.my_gsplat import TrackerConfig

    parser = Parser("Replica", "room0", normalize=True, input_folder=str(root))
    depth, rgb, pose = parser.frame(0)
    cfg = TrackerConfig(max_steps=ITERS)
    loc = Localizer(parser.K, W, H, cfg, mode="map", map_config=map_config)
    loc.reset(depth, rgb, pose)
    after_reset = loc.map.n_live
    gts, results, before = [pose], [], []
    for i in range(1, n_frames):
        depth, rgb, pose = parser.frame(i)
        before.append(loc.map.points.cpu().numpy().copy())
        results.append(loc.track(depth, rgb, gt_c2w=pose))
        gts.append(pose)
    K = parser.K.cpu()
    intr = (float(K[0, 0]), float(K[1, 1]), float(K[0, 2]), float(K[1, 2]))
    return dict(traj=loc.trajectory, gts=torch.stack(gts), results=results, after_reset=after_reset, loc=loc,
                before=before, intr=intr, near=cfg.gs.near_plane, far=cfg.gs.far_plane)


def _bits(run):
    return (run["traj"].cpu().numpy().view(np.uint32), [r.steps for r in run["results"]],
            [r.added for r in run["results"]])


@pytest.fixture(scope="module")
def seq_b(tmp_path_factory):
    root = tmp_path_factory.mktemp("view_seq_b")
    write_replica_constant_twist(root, W, H, N_B, rot_deg=0.4, trans=0.01)
    return root


@pytest.fixture(scope="module")
def sweep(tmp_path_factory):
    """The sweep's files, its ground-truth poses, the yardstick's pair errors and the uncut map-mode run."""
    root = tmp_path_factory.mktemp("view_sweep")
    poses = write_replica_constant_twist(root, W, H, N_SWEEP, rot_deg=SWEEP_DEG, trans=SWEEP_TRANS)
    return dict(root=root, poses=poses, eT=_yardstick(root, N_SWEEP), uncut=_run(root, N_SWEEP, MapConfig()))


def test_neutral_when_everything_is_in_view(seq_b, capsys):
    first, second = _run(seq_b, N_B, MapConfig()), _run(seq_b, N_B, MapConfig())
    culled = _run(seq_b, N_B, MapConfig(view_guard_px=10.0 * W))
    (p1, s1, a1), (p2, s2, a2), (pc, sc, ac) = _bits(first), _bits(second), _bits(culled)
    repeats = np.array_equal(p1, p2) and s1 == s2 and a1 == a2
    d_pose = float((first["traj"] - second["traj"]).abs().max())
    d_steps, d_added = max(abs(a - b) for a, b in zip(s1, s2)), max(abs(a - b) for a, b in zip(a1, a2))
    c_pose = float((first["traj"] - culled["traj"]).abs().max())
    c_steps, c_added = max(abs(a - b) for a, b in zip(s1, sc)), max(abs(a - b) for a, b in zip(a1, ac))
    with capsys.disabled():
        print(f"[view] (a) uncut twice: repeats bit for bit {repeats}; largest difference pose {d_pose:.3e}, steps "
              f"{d_steps}, added {d_added}; culled against the first uncut run: pose {c_pose:.3e}, steps {c_steps}, "
              f"added {c_added}; steps {s1} / {sc}, added {a1} / {ac}")
    for r in culled["results"]:
        assert r.tracked == r.map_size - r.added and r.view_violations == 0 and not r.lost
    assert all(r.view_violations is None and r.tracked == r.map_size - r.added for r in first["results"])
    if repeats:
        assert np.array_equal(pc, p1) and sc == s1 and ac == a1
    else:
        assert c_pose <= d_pose and c_steps <= d_steps and c_added <= d_added


def test_the_sweep_leaves_the_view(sweep):
    """The sequence is what the bounds assume: with ground-truth poses, frame 0's points and the guard, the mirror
    leaves at least a fifth of them out at the last pose, and none at the first."""
    run = sweep["uncut"]
    pts0 = run["before"][0]
    assert pts0.shape == (W * H, 3)
    share = [1.0 - ref.in_view(pts0, ref.w2c_of(p.numpy()), run["intr"], W, H, GUARD, run["near"], run["far"]).mean()
             for p in sweep["poses"]]
    print("[view] share of frame 0's points outside the guarded view per pose", ["%.3f" % s for s in share])
    assert share[0] == 0.0 and share[-1] >= 0.20 and all(b >= a for a, b in zip(share, share[1:]))


def _check_view_run(tag, sweep, run, guard, capsys):
    with capsys.disabled():
        _check_drift(tag, run, sweep["eT"])  # no frame lost, every frame under 2 sum eT_i
        print(f"[view] {tag}: tracked {[r.tracked for r in run['results']]}, violations "
              f"{[r.view_violations for r in run['results']]}")
    _check_growth(run)
    first_cut = None
    for k, (r, prefix) in enumerate(zip(run["results"], run["before"])):
        mask = ref.in_view(prefix, ref.w2c_of(r.init_c2w.cpu().numpy()), run["intr"], W, H, guard, run["near"],
                           run["far"])
        assert r.tracked == int(mask.sum()), (tag, k, r.tracked, int(mask.sum()))
        if first_cut is None and not mask.all():
            first_cut = k
        if first_cut is not None:
            assert r.tracked < len(prefix), (tag, k)
    assert first_cut is not None and first_cut <= N_SWEEP // 2, first_cut
    added, uncut = sum(r.added for r in run["results"]), sum(r.added for r in sweep["uncut"]["results"])
    with capsys.disabled():
        print(f"[view] {tag}: rows added {added}, uncut {uncut}; map rows {run['results'][-1].map_size} / "
              f"{sweep['uncut']['results'][-1].map_size}; first frame with a row left out {first_cut + 1}")
    assert added <= 1.5 * uncut, (added, uncut)


def test_the_uncut_mode_holds_on_the_sweep(sweep, capsys):
    """The sweep is not too hard for the tracker: the map mode without the option loses no frame and stays in its
    bounds on it (otherwise a failure below would say nothing about the local map)."""
    with capsys.disabled():
        _check_drift("sweep uncut", sweep["uncut"], sweep["eT"])
    _check_growth(sweep["uncut"])


def test_sweep_tracked_against_the_view(sweep, capsys):
    run = _run(sweep["root"], N_SWEEP, MapConfig(view_guard_px=GUARD))
    _check_view_run("sweep guard 8", sweep, run, GUARD, capsys)


def test_the_check_bites_at_the_smallest_guard(sweep, capsys):
    cfg = MapConfig(view_guard_px=MapConfig().view_reach_px)
    run = _run(sweep["root"], N_SWEEP, cfg)
    _check_view_run("sweep guard = reach", sweep, run, cfg.view_guard_px, capsys)
    assert any(r.view_violations > 0 for r in run["results"]), [r.view_violations for r in run["results"]]
