"""GPU: sequential localisation (gsplatloc_amd.localizer.Localizer, `python -m gsplatloc_amd.eval --sequential`) on two
synthetic Replica-format sequences of 6 frames at 160x120, tracked from the ground-truth pose of frame 0 only.

  A  write_replica_sequence: random-walk steps of 0.4 degrees / 1 cm;
  B  write_replica_constant_twist: the same twist every frame (0.4 degrees, 1 cm, fixed axis and direction).

Yardstick: the unchanged ground-truth-initialised protocol (evaluate_room without `sequential`) on the same files; its
per-pair errors eT_i are read from its --verbose lines (4 significant digits).  That is the parent's code path.

Drift: pair errors of this size compose linearly -- a rotation error acts on later frames through the 1 cm step, about
2e-6 m, not through the room -- so the absolute error at frame k is at most the sum of the pair errors before it.  The
sequential run starts every pair from another pose than the yardstick run, so each of its pair errors may differ from the
yardstick's: a factor 2.  Hence |t_k - gt_k| <= 2 sum_{i<k} eT_i.  On top, the final error is below a quarter of the
path length (a composition bug leaves errors of the size of the motion itself), and no frame is lost.

Prediction (B, constant velocity): every start pose from the third frame on is closer to ground truth than half the
inter-frame translation (second-order term |dt| theta = 7e-5 m against 1e-2 m, plus two estimate errors; "hold" starts
one whole step away)."""
import json
import re
import subprocess
import sys

import pytest
import torch

from gsplatloc_amd.synthetic import frame_pair, write_replica_constant_twist, write_replica_sequence

pytestmark = pytest.mark.gpu
DEV = "cuda"
W, H, N_FRAMES, ITERS = 160, 120, 6, 2000
STEP_T = 0.01


def _yardstick(root, capsys):
    """evaluate_room as it was (ground-truth placement and start): the per-pair translation errors."""
    from gsplatloc_amd.data import Parser
    from gsplatloc_amd.eval import evaluate_room

    capsys.readouterr()
    rep = evaluate_room(Parser("Replica", "room0", normalize=True, input_folder=str(root)), ITERS, None, verbose=True)
    lines = capsys.readouterr().out
    eT = [float(m) for m in re.findall(r"^frame \d+: .* eT (\S+) eR", lines, flags=re.M)]
    assert len(eT) == N_FRAMES - 1 == rep["frames_with_result"], (lines, rep)
    assert "mode" not in rep and "motion" not in rep  # the report of the existing protocol is what it was
    return eT, rep


def _sequential(root, motion):
    from gsplatloc_amd.data import Parser
    from gsplatloc_amd.localizer import Localizer
    from gsplatloc_amd.my_gsplat import TrackerConfig

    parser = Parser("Replica", "room0", normalize=True, input_folder=str(root))
    depth, rgb, pose = parser.frame(0)
    loc = Localizer(parser.K, W, H, TrackerConfig(max_steps=ITERS), motion=motion)
    loc.reset(depth, rgb, pose)
    gts, results = [pose], []
    for i in range(1, N_FRAMES):
        depth, rgb, pose = parser.frame(i)
        results.append(loc.track(depth, rgb, gt_c2w=pose))
        gts.append(pose)
    return loc.trajectory, torch.stack(gts), results


def _check_drift(tag, traj, gts, results, eT_pairs):
    err = (traj[:, :3, 3] - gts[:, :3, 3]).norm(dim=1).tolist()
    bounds = [2.0 * sum(eT_pairs[:k]) for k in range(N_FRAMES)]
    path = float((gts[1:, :3, 3] - gts[:-1, :3, 3]).norm(dim=1).sum())
    steps = [r.steps for r in results]
    print(f"[localizer] {tag}: abs error per frame {['%.3e' % e for e in err]}")
    print(f"[localizer] {tag}: bound 2 sum eT_i    {['%.3e' % b for b in bounds]}  (yardstick eT_i "
          f"{['%.3e' % e for e in eT_pairs]})")
    print(f"[localizer] {tag}: path {path:.4f} m, final error {err[-1]:.3e} m, mean steps {sum(steps) / len(steps):.1f}, "
          f"best steps {[r.best_step for r in results]}")
    assert err[0] == 0.0
    assert not any(r.lost for r in results), [r.best_step for r in results]
    for k in range(1, N_FRAMES):
        assert abs(results[k - 1].eT - err[k]) <= 1e-6
        assert err[k] <= bounds[k], (tag, k, err[k], bounds[k])
    assert err[-1] < 0.25 * path, (err[-1], path)


@pytest.fixture(scope="module")
def seq_a(tmp_path_factory):
    root = tmp_path_factory.mktemp("seq_a")
    write_replica_sequence(root, W, H, N_FRAMES)
    return root


@pytest.fixture(scope="module")
def seq_b(tmp_path_factory):
    root = tmp_path_factory.mktemp("seq_b")
    write_replica_constant_twist(root, W, H, N_FRAMES, rot_deg=0.4, trans=STEP_T)
    return root


def test_hold_drift_on_the_random_walk(seq_a, capsys):
    eT_pairs, rep = _yardstick(seq_a, capsys)
    traj, gts, results = _sequential(seq_a, "hold")
    for k, r in enumerate(results):  # "hold": every frame starts from the previous estimate
        assert torch.equal(r.init_c2w, traj[k])
    with capsys.disabled():
        _check_drift("A hold", traj, gts, results, eT_pairs)


def test_constant_velocity_prediction_and_drift_on_the_constant_twist(seq_b, capsys):
    eT_pairs, rep = _yardstick(seq_b, capsys)
    traj, gts, results = _sequential(seq_b, "constant_velocity")
    assert torch.equal(results[0].init_c2w, traj[0])  # the second frame has one estimate behind it: hold
    gaps = [float((results[k - 1].init_c2w[:3, 3] - gts[k][:3, 3]).norm()) for k in range(2, N_FRAMES)]
    _, _, held = _sequential(seq_b, "hold")
    with capsys.disabled():
        print(f"[localizer] B constant velocity: start pose off ground truth by {['%.3e' % g for g in gaps]} m "
              f"(half a step: {0.5 * STEP_T:.1e})")
        print(f"[localizer] B mean steps: constant velocity {sum(r.steps for r in results) / len(results):.1f}, "
              f"hold {sum(r.steps for r in held) / len(held):.1f}")
        for g in gaps:
            assert g < 0.5 * STEP_T, gaps
        _check_drift("B constant velocity", traj, gts, results, eT_pairs)


def test_best_c2w_of_both_trackers_agree():
    """TrackResult.best_c2w: GraphTracker (kept on the device by the pose step) against PoseTracker(engine="context")
    (kept by the host loop), on the frame pair and within the bounds test_graph_tracker_matches_pose_tracker uses for
    best_eT / best_eR (1e-4 m, 2e-3 degrees); and each one's own error against ground truth is its best_eT."""
    import gsplatloc_amd.my_gsplat as M
    from gsplatloc_amd.graph_tracker import GraphTracker
    from gsplatloc_amd.my_gsplat.trainer import calculate_rotation_error, calculate_translation_error

    fp = frame_pair(W, H, rot_deg=0.3, trans=0.01)
    K = fp["K"].to(DEV)
    pts0, pts1 = M.depth_to_points(fp["depth0"].to(DEV), K), M.depth_to_points(fp["depth1"].to(DEV), K)
    scales0 = M.init_gs_scales(pts0)
    rgb, c2w0, c2w1 = fp["rgb"].to(DEV), fp["c2w0"].to(DEV), fp["c2w1"].to(DEV)
    src_depth = M.compute_depth_gt(pts1, rgb, K[None], torch.eye(4, device=DEV)[None], H, W)[None, ..., None]
    cfg = M.TrackerConfig(max_steps=40, min_step=5, patience=1000)
    ref = M.PoseTracker(cfg, engine="context").track_frame(pts0, rgb, src_depth, c2w0, c2w1, K, W, H, scales=scales0)
    gt = GraphTracker(pts0.shape[0], W, H, cfg, device=DEV, poll=10)
    gt.load_frame(pts0, rgb, scales0, src_depth, c2w0, c2w1, K)
    res = gt.run()
    print(f"[localizer] best step: graph {res.best_step}, context {ref.best_step}; best eT {res.best_eT:.4e} / "
          f"{ref.best_eT:.4e}")
    assert res.best_step > cfg.min_step and ref.best_step > cfg.min_step
    assert res.best_c2w.shape == (4, 4) and ref.best_c2w.shape == (4, 4)
    assert calculate_translation_error(res.best_c2w, ref.best_c2w) < 1e-4
    assert calculate_rotation_error(res.best_c2w, ref.best_c2w) < 2e-3
    for r in (res, ref):
        assert abs(calculate_translation_error(r.best_c2w, c2w1) - r.best_eT) <= 1e-6
    # no minimum ever recorded: best_c2w is the last iterate
    short = M.TrackerConfig(max_steps=4, min_step=5, patience=1000)
    gt2 = GraphTracker(pts0.shape[0], W, H, short, device=DEV, poll=10)
    gt2.load_frame(pts0, rgb, scales0, src_depth, c2w0, c2w1, K)
    r2 = gt2.run()
    assert r2.best_step == -1 and torch.equal(r2.best_c2w, r2.final_c2w)


def test_sequential_cli(seq_a, tmp_path, repo_root):
    out = tmp_path / "res.json"
    cmd = [sys.executable, "-m", "gsplatloc_amd.eval", "--dataset", "Replica", "--rooms", "room0", "--root", str(seq_a),
           "--num-iters", str(ITERS), "--out", str(out), "--sequential"]
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=repo_root)
    assert res.returncode == 0, res.stderr[-3000:]
    r = json.loads(out.read_text())["room0"]["gsplatloc_amd"]
    print("[localizer] --sequential", json.dumps(r))
    assert set(r) >= {"mode", "motion", "ATE", "AAE", "final_eT", "final_eR", "path_length", "frames", "lost_frames",
                      "mean_steps", "seconds", "frames_per_s"}
    assert r["mode"] == "sequential" and r["motion"] == "constant_velocity" and r["frames"] == N_FRAMES - 1
    assert r["lost_frames"] == 0 and r["final_eT"] < 0.25 * r["path_length"]
