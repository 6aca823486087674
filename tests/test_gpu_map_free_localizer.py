"""GPU: Localizer(mode="map") with MapConfig.free_rho -- after every frame's insertion the rows of the map that the frame
sees through are removed -- at 160x120, "ED", with the settings and the yardstick of tests/test_gpu_map_localizer.py.

(a) The static room, the 6-frame constant twist of that file, free_rho = 0.05: nothing is removed on any frame, and
    poses, step counts and added rows are bit for bit those of free_rho = None run in the same process.  The map mode
    without removal is run twice first; if those two runs do not repeat bit for bit, the free run must lie within their
    difference (as tests/test_gpu_map_view_localizer.py does it).
(b) The vanishing panel (write_replica_vanishing_panel: 1 degree and 1 cm per frame, a panel of 0.4 x 0.3 m at z = 1.5 m,
    484 of frame 0's 19 200 pixels), 7 frames, the panel in frames 0 .. 2 and gone from frame 3, once with
    free_rho = None and once with free_rho = 0.05, window 1.  Panel rows are counted in host copies of the map: the rows
    within 1 cm of the panel's plane and inside its rectangle (widened by 1 cm).  No frame is lost in either run;
    frames 1 .. 3 are bit-identical between the runs (removal acts after tracking, and removes nothing while the panel
    is there: the numpy mirror gives 0 up to 7 mm / 0.05 degrees of pose error); frames 3 .. 6 together remove at least
    90 % of the panel rows and at most 10 % are left at the end (the mirror removes all 484 at frame 3 with poses up to
    30 mm / 0.3 degrees off); non-panel rows removed over the whole run are at most 0.5 % of the live rows (mirror: 0);
    without removal every panel row is still there at the end; the free run's frame 4 adds more rows than the other
    run's by at least a quarter of the pixels the panel covered at frame 3 -- the hole behind the ghost is filled by
    the frame after the removal (a 22 px hole less a ring of about 1 px in which the neighbours' alpha is still above
    alpha_min would be about 80 %); the final frame's absolute error is under the bound of the map test, twice the
    running sum of the ground-truth-start yardstick's pair errors on this sequence.  No ratio between the two runs'
    errors is asserted; the per-frame figures are printed.

Measured on the MI355X: (a) the two runs without removal repeat bit for bit -- steps 349, 648, 321, 572, 356, added rows
120, 120, 145, 135, 130 -- and the free run gives the same bits, removed 0 x 5.  (b) 508 panel rows before frame 3 in
both runs (frames 1 and 2 added 24); removed 0, 0, 508, 0, 0, 0: every panel row and no other; added 391, 459, 402, 906,
438, 439 against 391, 459, 402, 442, 396, 443 -- 464 more at frame 4 for 470 covered pixels; absolute error per frame
5.5e-4, 3.3e-4, 1.1e-3, 1.3e-3, 1.7e-3, 2.2e-3 m (without removal 5.5e-4, 3.3e-4, 1.1e-3, 1.3e-3, 2.3e-3, 2.2e-3) under a
bound of 1.9e-2 m at the last frame; no frame lost; without removal 508 panel rows at the end.  NOTES.md, "Free
space", has the 640x480 figures."""
import numpy as np
import pytest
import torch

from gsplatloc_amd.mapping import MapConfig
from gsplatloc_amd.synthetic import (panel_depth, replica_intrinsics, room_depth, write_replica_constant_twist,
                                     write_replica_vanishing_panel)
from tests.test_gpu_map_localizer import N_B, H, W, _yardstick
from tests.test_gpu_map_view_localizer import _bits, _run

pytestmark = pytest.mark.gpu
N_PANEL, N_WITH = 7, 3
CENTER, SIZE, Z_PANEL, TOL = (0.0, 0.0), (0.4, 0.3), 1.5, 0.01


def _panel_rows(points):
    """How many of the rows [n,3] (world) lie on the panel: within 1 cm of its plane, inside its rectangle."""
    p = np.asarray(points, dtype=np.float64)
    on = (np.abs(p[:, 2] - Z_PANEL) <= TOL) & (np.abs(p[:, 0] - CENTER[0]) <= SIZE[0] / 2 + TOL) \
        & (np.abs(p[:, 1] - CENTER[1]) <= SIZE[1] / 2 + TOL)
    return int(on.sum())


def test_nothing_is_removed_from_the_static_room(tmp_path, capsys):
    write_replica_constant_twist(tmp_path, W, H, N_B, rot_deg=0.4, trans=0.01)
    first, second = _run(tmp_path, N_B, MapConfig()), _run(tmp_path, N_B, MapConfig())
    free = _run(tmp_path, N_B, MapConfig(free_rho=0.05))
    (p1, s1, a1), (p2, s2, a2), (pf, sf, af) = _bits(first), _bits(second), _bits(free)
    repeats = np.array_equal(p1, p2) and s1 == s2 and a1 == a2
    d_pose = float((first["traj"] - second["traj"]).abs().max())
    d_steps, d_added = max(abs(a - b) for a, b in zip(s1, s2)), max(abs(a - b) for a, b in zip(a1, a2))
    f_pose = float((first["traj"] - free["traj"]).abs().max())
    f_steps, f_added = max(abs(a - b) for a, b in zip(s1, sf)), max(abs(a - b) for a, b in zip(a1, af))
    with capsys.disabled():
        print(f"[free] (a) without removal twice: repeats bit for bit {repeats}; largest difference pose {d_pose:.3e}, "
              f"steps {d_steps}, added {d_added}; free_rho 0.05 against the first: pose {f_pose:.3e}, steps {f_steps}, "
              f"added {f_added}; steps {s1} / {sf}, added {a1} / {af}, removed {[r.removed for r in free['results']]}")
    assert all(r.removed is None for r in first["results"])
    assert [r.removed for r in free["results"]] == [0] * (N_B - 1) and not any(r.lost for r in free["results"])
    assert all(r.map_size == r.tracked + r.added for r in free["results"])
    if repeats:
        assert np.array_equal(pf, p1) and sf == s1 and af == a1
    else:
        assert f_pose <= d_pose and f_steps <= d_steps and f_added <= d_added


def test_a_panel_that_vanishes_is_removed_and_the_hole_is_filled(tmp_path, capsys):
    poses = write_replica_vanishing_panel(tmp_path, W, H, N_PANEL, N_WITH, center=CENTER, size=SIZE, z=Z_PANEL)
    eT_pairs = _yardstick(tmp_path, N_PANEL)
    none, free = _run(tmp_path, N_PANEL, MapConfig()), _run(tmp_path, N_PANEL, MapConfig(free_rho=0.05, free_window_px=1))
    K = replica_intrinsics(W, H)
    at3 = poses[N_WITH].float()
    covered = int((panel_depth(W, H, K, at3, CENTER, SIZE, Z_PANEL) < room_depth(W, H, K, at3)).sum())
    fig = {}
    for tag, run in (("none", none), ("free", free)):
        res = run["results"]
        err = (run["traj"][:, :3, 3] - run["gts"][:, :3, 3]).norm(dim=1).tolist()
        # run["before"][k]: the live rows before frame k + 1 is tracked
        fig[tag] = dict(err=err, before3=_panel_rows(run["before"][N_WITH - 1]),
                        end=_panel_rows(run["loc"].map.points.cpu().numpy()), added=[r.added for r in res],
                        removed=[r.removed for r in res], steps=[r.steps for r in res], live=run["loc"].map.n_live)
    bounds = [2.0 * sum(eT_pairs[:k]) for k in range(N_PANEL)]
    with capsys.disabled():
        for tag in ("none", "free"):
            f = fig[tag]
            print(f"[free] (b) {tag}: abs error per frame {['%.3e' % e for e in f['err']]}, steps {f['steps']}, added "
                  f"{f['added']}, removed {f['removed']}, panel rows before frame 3 {f['before3']}, at the end "
                  f"{f['end']}, live rows {f['live']}")
        print(f"[free] (b) bound 2 sum eT_i {['%.3e' % b for b in bounds]}; pixels the panel covered at frame 3: {covered}")
    n, f = fig["none"], fig["free"]
    assert not any(r.lost for r in none["results"]) and not any(r.lost for r in free["results"])
    assert all(r.removed is None for r in none["results"])
    # frames 1 .. 3: the same bits (the removal acts after tracking and removes nothing while the panel is there)
    assert np.array_equal(none["traj"][:N_WITH + 1].cpu().numpy().view(np.uint32),
                          free["traj"][:N_WITH + 1].cpu().numpy().view(np.uint32))
    assert n["steps"][:N_WITH] == f["steps"][:N_WITH] and n["added"][:N_WITH] == f["added"][:N_WITH]
    assert f["removed"][:N_WITH - 1] == [0] * (N_WITH - 1)
    # the panel was in the map, and goes once it is gone from the frames
    panel = f["before3"]
    assert panel == n["before3"] and 0.9 * 484 <= panel <= 1.2 * 484, (panel, n["before3"])
    gone = sum(f["removed"][N_WITH - 1:])
    assert gone >= 0.9 * panel and f["end"] <= 0.1 * panel, (f["removed"], f["end"], panel)
    assert sum(f["removed"]) - (panel - f["end"]) <= 0.005 * f["live"], (f["removed"], panel, f["end"], f["live"])
    assert n["end"] == n["before3"]  # without removal the ghost stays
    # the hole is filled by the frame after the removal
    assert f["added"][N_WITH] - n["added"][N_WITH] >= covered / 4, (f["added"], n["added"], covered)
    # drift: the last frame under the bound of the map test
    assert f["err"][-1] <= bounds[-1], (f["err"], bounds)
    assert f["live"] == W * H + sum(f["added"]) - sum(f["removed"])


def test_the_evaluation_driver_reports_the_removed_rows(tmp_path):
    """evaluate_room(sequential, map_mode, map_free_rho): the report gains removed_per_frame, and the counts add up."""
    from gsplatloc_amd.data import Parser
    from gsplatloc_amd.eval import evaluate_room
    from tests.test_gpu_map_localizer import ITERS

    write_replica_vanishing_panel(tmp_path, W, H, 5, 2, center=CENTER, size=SIZE, z=Z_PANEL)
    parser = Parser("Replica", "room0", normalize=True, input_folder=str(tmp_path))
    r = evaluate_room(parser, ITERS, None, sequential=True, map_mode=True, map_free_rho=0.05, map_free_window=1)
    assert r["free_rho"] == 0.05 and r["free_window_px"] == 1 and r["lost_frames"] == 0 and r["frames"] == 4
    assert len(r["removed_per_frame"]) == 4 and r["removed_per_frame"][0] == 0 and sum(r["removed_per_frame"]) >= 0.9 * 484
    assert r["map_gaussians"] == W * H + sum(r["added_per_frame"]) - sum(r["removed_per_frame"])
    plain = evaluate_room(parser, ITERS, None, sequential=True, map_mode=True)
    assert "removed_per_frame" not in plain and "free_rho" not in plain
    assert plain["map_gaussians"] == W * H + sum(plain["added_per_frame"])
