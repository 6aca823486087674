"""GPU: Localizer(mode="map") with ``MapConfig.refine`` at 160x120, with the settings and the yardstick of
tests/test_gpu_map_localizer.py (the ground-truth-initialised protocol on the same files; |t_k - gt_k| <= 2 sum_{i<k}
eT_i, no frame lost).

  (a) the constant twist of that file (6 frames, 0.4 degrees and 1 cm a frame, noise-free), the real tracker, refine on:
      no frame is lost, every frame refines rows, every frame is inside the bound; and a run with ``refine=False`` is
      the run with a default MapConfig bit for bit (nothing new is allocated or launched).
  (b) the noisy sequence of tests/test_map_refine_cpu.py (9 frames, sigma = 5 mm), a stand-in tracker that answers the
      exact pose, the real map kernels and the real insertion render: the RMS distance to the box's planes of the rows
      that all 8 frames refined well inside their four pixels falls to at most a half (the expectation is a third: the
      mean of 9 samples), and those rows are at least a quarter of frame 0's.
  (c) the noisy sequence written as files, the real tracker, with the option and twice without it: no frame is lost
      and every frame is inside the bound of the noisy files' own yardstick.  The three ATEs are printed, not compared:
      nobody has measured the one against the others (NOTES.md, "Refinement", has the figures of one run)."""
import numpy as np
import pytest
import torch

from gsplatloc_amd.localizer import Localizer
from gsplatloc_amd.mapping import MapConfig
from gsplatloc_amd.my_gsplat import TrackerConfig
from gsplatloc_amd.synthetic import _twist, _write_replica_poses, replica_intrinsics, room_depth, write_replica_constant_twist
from tests import map_refine_ref as ref
from tests import test_map_refine_cpu as cpu
from tests.test_gpu_map_localizer import ITERS, N_B, H, W, _check_drift, _yardstick
from tests.test_map_cpu import _Tracker

pytestmark = pytest.mark.gpu
assert (W, H) == (cpu.NW, cpu.NH)
N_NOISY = cpu.N_REFINE + 1


def _run(root, n_frames, config):
    from gsplatloc_amd.data import Parser

    parser = Parser("Replica", "room0", normalize=True, input_folder=str(root))
    depth, rgb, pose = parser.frame(0)
    loc = Localizer(parser.K, W, H, TrackerConfig(max_steps=ITERS), mode="map", map_config=config)
    loc.reset(depth, rgb, pose)
    gts, results = [pose], []
    for i in range(1, n_frames):
        depth, rgb, pose = parser.frame(i)
        results.append(loc.track(depth, rgb, gt_c2w=pose))
        gts.append(pose)
    return dict(traj=loc.trajectory, gts=torch.stack(gts), results=results, loc=loc)


def _ate(run):
    e = (run["traj"][1:, :3, 3] - run["gts"][1:, :3, 3].to(run["traj"].device)).norm(dim=1)
    return float(e.square().mean().sqrt())


@pytest.fixture(scope="module")
def seq_b(tmp_path_factory):
    root = tmp_path_factory.mktemp("refine_seq_b")
    write_replica_constant_twist(root, W, H, N_B, rot_deg=0.4, trans=0.01)
    return root


@pytest.fixture(scope="module")
def seq_noisy(tmp_path_factory):
    """The twist of ``cpu.noisy_sequence`` in the Replica layout, every depth image with its own noise (what the file
    keeps of it: 1 / 6553.5 m steps)."""
    root = tmp_path_factory.mktemp("refine_seq_noisy")
    step, c2w, poses = _twist(0.4, 0.01, (0.3, 1.0, -0.2), (0.6, 0.1, 0.8)), np.eye(4), []
    for i in range(N_NOISY):
        if i:
            c2w = c2w @ step
        poses.append(c2w.copy())
    rng = np.random.default_rng(0)

    def depth_of(i, K, pose):
        return room_depth(W, H, K, pose) + torch.from_numpy((cpu.SIGMA * rng.standard_normal((H, W))).astype(np.float32))

    _write_replica_poses(root, W, H, poses, depth_of)
    return root


def test_refinement_on_the_constant_twist(seq_b, capsys):
    eT_pairs = _yardstick(seq_b, N_B)
    run = _run(seq_b, N_B, MapConfig(refine=True))
    with capsys.disabled():
        err = _check_drift("B map refine", run, eT_pairs)
        print(f"[refine] B: rows refined per frame {[r.refined for r in run['results']]}")
    assert all(r.refined > 0 for r in run["results"])
    weights = run["loc"].map.weights[:W * H]
    assert int(weights.max()) == N_B and int(weights.min()) >= 1
    # the option off is the default: nothing of it is allocated or launched, and the run is the same in every bit
    off, plain = _run(seq_b, N_B, MapConfig(refine=False)), _run(seq_b, N_B, MapConfig())
    assert off["loc"].map.weights is None and all(r.refined is None for r in off["results"])
    assert torch.equal(off["traj"], plain["traj"])
    assert [(r.steps, r.added, r.best_loss) for r in off["results"]] == [(r.steps, r.added, r.best_loss)
                                                                         for r in plain["results"]]
    assert torch.equal(off["loc"].map.points, plain["loc"].map.points)
    with capsys.disabled():
        plain_err = _check_drift("B map", plain, eT_pairs)
        print(f"[refine] B: ATE with refinement {_ate(run):.3e} m, without {_ate(plain):.3e} m; final error "
              f"{err[-1]:.3e} / {plain_err[-1]:.3e} m")


def test_the_device_averages_the_depth_noise_away(capsys):
    frames = cpu.noisy_sequence()
    K = replica_intrinsics(W, H)
    intr = tuple(float(np.float32(a)) for a in (K[0, 0], K[1, 1], K[0, 2], K[1, 2]))
    _Tracker.made = []
    loc = Localizer(K, W, H, TrackerConfig(max_steps=5), normalize=False, motion="hold", tracker_factory=_Tracker,
                    mode="map", map_config=MapConfig(refine=True))
    loc.reset(frames[0][0], None, frames[0][1])
    n = W * H
    assert loc.map.n_live == n
    before = loc.map.points.cpu().numpy().copy()
    refined = []
    for depth, pose in frames[1:]:
        last = loc.map.means[:n].cpu().numpy().copy()  # frame 0's rows as this frame finds them
        r = loc.track(depth, None, gt_c2w=pose)
        assert not r.lost and float((r.c2w.cpu() - pose).abs().max()) <= 1e-6  # the stand-in answers the exact pose
        refined.append(r.refined)
    after, weights = loc.map.means[:n].cpu().numpy(), loc.map.weights[:n].cpu().numpy()
    # where the last frame saw the rows: the mirror's projection of the rows it found, at its pose
    _, u, v = ref.project(last, ref.w2c_of(frames[-1][1].numpy()), intr)
    with np.errstate(invalid="ignore"):
        a = u - np.minimum(np.floor(u), W - 2).astype(np.float32)
        b = v - np.minimum(np.floor(v), H - 2).astype(np.float32)
    ratio, share = cpu.noise_verdict(before, after, weights, a, b)
    with capsys.disabled():
        print(f"[refine] device, {cpu.N_REFINE} frames of {cpu.SIGMA * 1e3:g} mm noise: RMS to the planes x {ratio:.3f} "
              f"over {share:.1%} of frame 0's rows; refined per frame {refined}, map {loc.map.n_live}")
    assert share >= 0.25
    assert ratio <= 0.5


def test_refinement_on_the_noisy_sequence(seq_noisy, capsys):
    eT_pairs = _yardstick(seq_noisy, N_NOISY)
    runs = {"refine": _run(seq_noisy, N_NOISY, MapConfig(refine=True)),
            "plain 1": _run(seq_noisy, N_NOISY, MapConfig()), "plain 2": _run(seq_noisy, N_NOISY, MapConfig())}
    with capsys.disabled():
        for tag, run in runs.items():
            _check_drift(f"noisy {tag}", run, eT_pairs)  # no frame lost, every frame inside the bound
        ates = {tag: _ate(run) for tag, run in runs.items()}
        print(f"[refine] noisy: ATE {', '.join(f'{t} {e:.4e} m' for t, e in ates.items())}; spread of the two plain runs "
              f"{abs(ates['plain 1'] - ates['plain 2']):.2e} m; refined per frame "
              f"{[r.refined for r in runs['refine']['results']]}")
    assert all(r.refined > 0 for r in runs["refine"]["results"])
