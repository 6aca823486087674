"""GPU: frame-to-map localisation (Localizer(mode="map"), `python -m gsplatloc_amd.eval --sequential --map`) at 160x120
with the iteration budget of tests/test_gpu_localizer.py, on

  B  write_replica_constant_twist, 6 frames: the same twist every frame (0.4 degrees, 1 cm);
  C  write_replica_there_and_back, 5 steps of that twist out and the same 5 poses back (11 frames).

Yardstick, as in tests/test_gpu_localizer.py: the unchanged ground-truth-initialised protocol (evaluate_room without
`sequential`) on the same files, its per-pair errors eT_i read from its --verbose lines.  The bound is that file's, with
its reasoning: pair errors of this size compose linearly and a run that starts every pair elsewhere may make each of them
up to twice as large, so |t_k - gt_k| <= 2 sum_{i<k} eT_i -- a map that works stays inside the frame-to-frame drift
budget; the final error is below a quarter of the path; no frame is lost.

Map growth on C is a condition, not a measurement: with the float64 oracle at 80x60 and ground-truth poses every outward
step of this twist selects 1.3 - 4 % of the pixels (a border column per step), every return frame 0.00 - 0.06 %, so the
rows added over the return half are about 2 % of those added on the way out; the cap here is a quarter.

Figures of the run these bounds were first checked with (MI355X): see NOTES.md, "Frame-to-map localisation"."""
import contextlib
import io
import json
import re
import subprocess
import sys

import pytest
import torch

from gsplatloc_amd.synthetic import write_replica_constant_twist, write_replica_there_and_back

pytestmark = pytest.mark.gpu
W, H, ITERS = 160, 120, 2000
N_B, N_OUT = 6, 5


def _yardstick(root, n_frames):
    """evaluate_room as it was (ground-truth placement and start): the per-pair translation errors."""
    from gsplatloc_amd.data import Parser
    from gsplatloc_amd.eval import evaluate_room

    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        rep = evaluate_room(Parser("Replica", "room0", normalize=True, input_folder=str(root)), ITERS, None, verbose=True)
    eT = [float(m) for m in re.findall(r"^frame \d+: .* eT (\S+) eR", out.getvalue(), flags=re.M)]
    assert len(eT) == n_frames - 1 == rep["frames_with_result"], (out.getvalue(), rep)
    return eT


def _run(root, n_frames, mode):
    from gsplatloc_amd.data import Parser
    from gsplatloc_amd.localizer import Localizer
    from gsplatloc_amd.my_gsplat import TrackerConfig

    parser = Parser("Replica", "room0", normalize=True, input_folder=str(root))
    depth, rgb, pose = parser.frame(0)
    loc = Localizer(parser.K, W, H, TrackerConfig(max_steps=ITERS), mode=mode)
    loc.reset(depth, rgb, pose)
    after_reset = loc.map.n_live if mode == "map" else None
    gts, results = [pose], []
    for i in range(1, n_frames):
        depth, rgb, pose = parser.frame(i)
        results.append(loc.track(depth, rgb, gt_c2w=pose))
        gts.append(pose)
    return dict(traj=loc.trajectory, gts=torch.stack(gts), results=results, after_reset=after_reset, loc=loc)


def _check_drift(tag, run, eT_pairs):
    traj, gts, results = run["traj"], run["gts"], run["results"]
    n = traj.shape[0]
    err = (traj[:, :3, 3] - gts[:, :3, 3]).norm(dim=1).tolist()
    bounds = [2.0 * sum(eT_pairs[:k]) for k in range(n)]
    path = float((gts[1:, :3, 3] - gts[:-1, :3, 3]).norm(dim=1).sum())
    print(f"[map] {tag}: abs error per frame {['%.3e' % e for e in err]}")
    print(f"[map] {tag}: bound 2 sum eT_i    {['%.3e' % b for b in bounds]}  (yardstick eT_i "
          f"{['%.3e' % e for e in eT_pairs]})")
    print(f"[map] {tag}: path {path:.4f} m, final error {err[-1]:.3e} m, steps {[r.steps for r in results]}, "
          f"added {[r.added for r in results]}, map {[r.map_size for r in results]}")
    assert err[0] == 0.0
    assert not any(r.lost for r in results), [r.best_step for r in results]
    for k in range(1, n):
        assert abs(results[k - 1].eT - err[k]) <= 1e-6
        assert err[k] <= bounds[k], (tag, k, err[k], bounds[k])
    assert err[-1] < 0.25 * path, (err[-1], path)
    return err


def _check_growth(run):
    results = run["results"]
    assert run["after_reset"] == W * H  # every pixel of frame 0: the room has no invalid depth
    sizes = [run["after_reset"]] + [r.map_size for r in results]
    assert all(b >= a for a, b in zip(sizes, sizes[1:])), sizes
    assert all(r.added >= 0 for r in results)
    assert sizes[-1] == W * H + sum(r.added for r in results) == run["loc"].map.n_live
    assert [b - a for a, b in zip(sizes, sizes[1:])] == [r.added for r in results]
    assert not run["loc"].map.full


@pytest.fixture(scope="module")
def seq_b(tmp_path_factory):
    root = tmp_path_factory.mktemp("map_seq_b")
    write_replica_constant_twist(root, W, H, N_B, rot_deg=0.4, trans=0.01)
    return root


@pytest.fixture(scope="module")
def seq_c(tmp_path_factory):
    root = tmp_path_factory.mktemp("map_seq_c")
    poses = write_replica_there_and_back(root, W, H, N_OUT, rot_deg=0.4, trans=0.01)
    assert poses.shape[0] == 2 * N_OUT + 1
    return root


@pytest.fixture(scope="module")
def there_and_back(seq_c):
    """The yardstick and the map-mode run on C, shared by the two tests that read them."""
    n = 2 * N_OUT + 1
    return _yardstick(seq_c, n), _run(seq_c, n, "map")


def test_map_mode_on_the_constant_twist(seq_b, capsys):
    eT_pairs = _yardstick(seq_b, N_B)
    run = _run(seq_b, N_B, "map")
    with capsys.disabled():
        _check_drift("B map", run, eT_pairs)
    _check_growth(run)


def test_map_mode_there_and_back(there_and_back, capsys):
    eT_pairs, run = there_and_back
    with capsys.disabled():
        _check_drift("C map", run, eT_pairs)
    _check_growth(run)
    added = [r.added for r in run["results"]]
    out, back = sum(added[:N_OUT]), sum(added[N_OUT:])
    with capsys.disabled():
        print(f"[map] C: rows added on the way out {out}, on the way back {back}")
    assert out > 0 and 4 * back <= out, (added, out, back)


def test_drift_on_return_against_frame_mode(seq_c, there_and_back, capsys):
    """Frame mode and map mode on the same files.  The final error on return in map mode must not exceed frame mode's by
    more than the spread of the drift bound: <= max(frame mode's final error, 2 sum eT_i).  How much smaller it is, is
    printed, not asserted."""
    eT_pairs, run = there_and_back
    frame = _run(seq_c, 2 * N_OUT + 1, "frame")
    assert all(r.added is None and r.map_size is None for r in frame["results"])

    def final(r):
        return float((r["traj"][-1, :3, 3] - r["gts"][-1, :3, 3]).norm())

    e_map, e_frame, budget = final(run), final(frame), 2.0 * sum(eT_pairs)
    with capsys.disabled():
        print(f"[map] C final error on return: map mode {e_map:.3e} m, frame mode {e_frame:.3e} m, "
              f"2 sum eT_i {budget:.3e} m; mean steps map {sum(r.steps for r in run['results']) / 10:.1f}, "
              f"frame {sum(r.steps for r in frame['results']) / 10:.1f}")
    assert not any(r.lost for r in frame["results"])
    assert e_map <= max(e_frame, budget), (e_map, e_frame, budget)


def test_sequential_map_cli(seq_b, tmp_path, repo_root):
    out = tmp_path / "res.json"
    cmd = [sys.executable, "-m", "gsplatloc_amd.eval", "--dataset", "Replica", "--rooms", "room0", "--root", str(seq_b),
           "--num-iters", str(ITERS), "--out", str(out), "--sequential", "--map"]
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=repo_root)
    assert res.returncode == 0, res.stderr[-3000:]
    r = json.loads(out.read_text())["room0"]["gsplatloc_amd"]
    print("[map] --sequential --map", json.dumps(r))
    assert set(r) >= {"mode", "motion", "ATE", "AAE", "final_eT", "final_eR", "path_length", "frames", "lost_frames",
                      "mean_steps", "seconds", "frames_per_s", "map_gaussians", "added_per_frame", "map_full"}
    assert r["mode"] == "sequential" and r["frames"] == N_B - 1 and r["lost_frames"] == 0
    assert r["map_full"] is False and len(r["added_per_frame"]) == N_B - 1
    assert r["map_gaussians"] == W * H + sum(r["added_per_frame"])
