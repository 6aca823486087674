"""GPU: Localizer(mode="map") with MapConfig.loop -- loops closed in track() -- on real kernels.

(a) The room loop (tests/map_correct_ref.room_loop): eight 160 x 120 frames of the box room, the camera on a 10 cm
    circle looking at a corner, the tracker's trajectory drifting by 0.3 degrees and 5 mm a frame.  A real
    ``GaussianMap``, the real renderer, and tests/test_map_cpu._Tracker as the tracker: it answers the pose it is handed
    as ground truth, so ``gt_c2w = est[k]`` scripts the drift.  ``loop_min_gap=7, loop_every=1``: for frame 7 the old
    frames are frame 0 alone -- the constraint tests/test_gpu_map_correct.py measures at 6e-6 m.  Frames 1 .. 6 find no
    old frame (``few_rows``); frame 7 closes the loop by itself with the anchor 0, lands within 2e-3 m and 2e-3
    (Frobenius, rotation) of its true pose -- the bound that test holds the same alignment to -- and the RMS distance of
    the rows from where the true poses put them falls to a half or less.  Then a second lap of eight, drifting on from
    the corrected pose: a second closure happens, and every kept edge is satisfied to 1e-5 (rad and m) after it.
(b) No drift, the real tracker: the 6-frame constant twist of tests/test_gpu_map_view_localizer.py, once with
    ``MapConfig(origins=True)`` and once with the loop policy on (``loop_min_gap=3, loop_every=1``).  No loop is closed,
    and poses and rows are bit for bit those of the run without the option."""
import numpy as np
import pytest
import torch

from gsplatloc_amd.localizer import Localizer
from gsplatloc_amd.mapping import MapConfig
from gsplatloc_amd.my_gsplat import TrackerConfig
from gsplatloc_amd.synthetic import replica_intrinsics, room_depth, write_replica_constant_twist
from tests import map_correct_ref as ref
from tests import test_map_cpu as base

pytestmark = pytest.mark.gpu
DEV = "cuda"
W, H = 160, 120
K = replica_intrinsics(W, H)
inv = np.linalg.inv


def _errors(pose, truth):
    pose, truth = np.asarray(pose, np.float64), np.asarray(truth, np.float64)
    return (float(np.linalg.norm(pose[:3, 3] - truth[:3, 3])), float(np.sqrt(((pose[:3, :3] - truth[:3, :3]) ** 2).sum())))


def test_the_localizer_closes_the_room_loop_by_itself(capsys):
    true, est = ref.room_loop()
    step_error = ref.twist(0.3, 0.005)  # what room_loop's drifted trajectory adds to every motion
    depths = [room_depth(W, H, K, torch.from_numpy(p).float()) for p in true]
    cfg = MapConfig(origins=True, loop=True, loop_min_gap=7, loop_every=1)
    base._Tracker.made = []
    loc = Localizer(K, W, H, TrackerConfig(max_steps=5), normalize=False, motion="hold", device=DEV,
                    tracker_factory=base._Tracker, mode="map", map_config=cfg)
    loc.reset(depths[0], None, torch.from_numpy(est[0]).float())
    inserted_at = [est[0]]  # the pose every frame's rows were written at
    results = []
    for k in range(1, 7):
        results.append(loc.track(depths[k], None, gt_c2w=torch.from_numpy(est[k]).float()))
        inserted_at.append(loc.trajectory[k].cpu().double().numpy())
    assert [r.loop_status for r in results] == ["few_rows"] * 6 and not any(r.loop or r.lost for r in results)
    assert all(r.loop_old_tested == 0 and r.added > 0 for r in results)
    n, o = loc.map.n_live, loc.map.origins[:loc.map.n_live].cpu().numpy()
    rows = loc.map.points.cpu().numpy().astype(np.float64)
    move = true[:7] @ inv(np.stack(inserted_at))  # per frame: from where its drifted pose put a row to where the true one does
    truth = np.einsum("nij,nj->ni", move[o, :3, :3], rows) + move[o, :3, 3]
    r = loc.track(depths[7], None, gt_c2w=torch.from_numpy(est[7]).float())
    err_t, err_r = _errors(loc.trajectory[7].cpu(), true[7])
    was_t, was_r = _errors(est[7], true[7])
    after = loc.map.points[:n].cpu().numpy().astype(np.float64)
    e0, e1 = ref.rms(rows - truth), ref.rms(after - truth)
    g = loc.last_pose_graph
    with capsys.disabled():
        print(f"[loop] frame 7: {r.loop_status}, anchor {r.loop_anchor}, old rows tested {r.loop_old_tested}, moved "
              f"{r.loop_moved_t:.3e} m {r.loop_moved_r_deg:.3e} deg; pose {was_t:.3e} m / {was_r:.3e} -> {err_t:.3e} m / "
              f"{err_r:.3e}; rows RMS {e0:.4f} m -> {e1:.4f} m, x {e1 / e0:.3f}; graph {g.iterations} iterations, cost "
              f"{g.cost_before:.3e} -> {g.cost_after:.3e}, edge residual {g.loop_residuals[0]:.2e}; "
              f"{r.loop_correction.moved} rows moved")
    assert r.loop is True and r.loop_status == "closed" and r.loop_anchor == 0 and not r.lost
    assert r.loop_old_tested == W * H  # every row of frame 0 is tested from the drifted pose
    assert err_t <= 2e-3 and err_r <= 2e-3
    assert torch.equal(r.c2w, loc.trajectory[7])
    assert e1 <= 0.5 * e0
    assert r.loop_correction.moved == n - W * H and r.loop_correction.outside == 0 and r.loop_correction.frames == 7
    assert np.array_equal(loc.map.points[:W * H].cpu().numpy(), rows[:W * H].astype(np.float32))  # frame 0 is held
    assert (loc.map.origins[n:loc.map.n_live] == 7).all()
    # a second lap: the drift goes on from the corrected pose
    closures, lines = [], []
    for k in range(8, 16):
        at = loc.trajectory[k - 1].cpu().double().numpy() @ inv(true[(k - 1) % 8]) @ true[k % 8] @ step_error
        r = loc.track(depths[k % 8], None, gt_c2w=torch.from_numpy(at).float())
        line = f"[loop] frame {k}: {r.loop_status}, old rows tested {r.loop_old_tested}"
        if r.loop:
            res = loc.last_pose_graph.loop_residuals
            closures.append((k, r.loop_anchor, float(res.max())))
            t, rot = _errors(loc.trajectory[k].cpu(), true[k % 8])
            line += (f", anchor {r.loop_anchor}, moved {r.loop_moved_t:.3e} m {r.loop_moved_r_deg:.3e} deg, {len(res)} edges, "
                     f"largest residual {res.max():.2e}, pose {t:.3e} m / {rot:.3e} from the truth")
        lines.append(line)
        assert not r.lost and r.loop_status in ("closed", "small", "rejected", "not_converged")
    with capsys.disabled():
        print("\n".join(lines))
    assert closures, "no second closure on the second lap"
    assert closures[0][2] <= 1e-5, closures  # every kept edge after the second closure
    assert len(loc._loops) == 1 + len(closures) and len(loc._odometry) == 15


def test_without_drift_no_loop_is_closed_and_nothing_changes(tmp_path_factory, capsys):
    from tests.test_gpu_map_view_localizer import _run

    root = tmp_path_factory.mktemp("loop_seq")
    write_replica_constant_twist(root, W, H, 6, rot_deg=0.4, trans=0.01)
    plain = _run(root, 6, MapConfig(origins=True))
    loop = _run(root, 6, MapConfig(origins=True, loop=True, loop_min_gap=3, loop_every=1))
    status = [r.loop_status for r in loop["results"]]
    with capsys.disabled():
        print(f"[loop] no drift: {status}, old rows tested {[r.loop_old_tested for r in loop['results']]}, moved "
              f"{[None if r.loop_moved_t is None else round(r.loop_moved_t, 6) for r in loop['results']]} m")
    assert all(r.loop is None and r.loop_status is None for r in plain["results"])
    assert all(r.loop is False for r in loop["results"]) and "closed" not in status and status[:2] == ["few_rows"] * 2
    assert loop["loc"]._loops == [] and len(loop["loc"]._odometry) == 5
    assert torch.equal(loop["traj"], plain["traj"])
    assert [r.steps for r in loop["results"]] == [r.steps for r in plain["results"]]
    assert [r.added for r in loop["results"]] == [r.added for r in plain["results"]]
    a, b = loop["loc"].map, plain["loc"].map
    assert a.n_live == b.n_live and torch.equal(a.points, b.points) and torch.equal(a.point_colors, b.point_colors)
    assert torch.equal(a.origins[:a.n_live], b.origins[:b.n_live])


def test_the_evaluation_driver_reports_the_closures(tmp_path_factory, capsys):
    from gsplatloc_amd.data import Parser
    from gsplatloc_amd.eval import evaluate_room
    from tests.test_gpu_map_localizer import ITERS

    root = tmp_path_factory.mktemp("loop_eval_seq")
    write_replica_constant_twist(root, W, H, 6, rot_deg=0.4, trans=0.01)
    parser = Parser("Replica", "room0", normalize=True, input_folder=str(root))
    r = evaluate_room(parser, ITERS, None, sequential=True, map_mode=True, map_loop=True, map_loop_min_gap=3)
    with capsys.disabled():
        print(f"[loop] evaluation driver: {r['loop_status_per_frame']}, ATE {r['ATE']:.3e} m, corrected {r['ate_corrected']:.3e} m")
    assert r["loop"] is True and r["origins"] is True and r["origins_non_decreasing"] is True  # the option implies them
    # loop_every is the default's 10: five frames wait
    assert r["loop_status_per_frame"] == ["waiting"] * 5 and r["frames"] == 5
    assert r["loop_closures"] == [] and r["loop_anchors"] == [] and r["loop_edge_residuals"] == []
    assert abs(r["ate_corrected"] - r["ATE"]) <= 1e-6  # nothing was corrected
    plain = evaluate_room(parser, ITERS, None, sequential=True, map_mode=True)
    assert "loop" not in plain and "loop_closures" not in plain and plain["ATE"] == r["ATE"]
