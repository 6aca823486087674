"""GPU: Localizer(mode="map") with MapConfig.info, on the sequence and with the settings of
tests/test_gpu_map_localizer.py -- write_replica_constant_twist at 160x120, 6 frames, 0.4 degrees and 1 cm per frame,
2000 iterations at the most.  The option reads the map and the depth image and writes neither: with it the trajectory,
the step counts, the rows added and every bit of the map are those of the run without it.  Every frame of this sequence
looks into the room's corners: none is weak, and each has a symmetric positive-definite covariance.  sigma_t is printed
beside the frame's true error eT and not held against it (NOTES.md, "Pose information").  And the frame of one plane of
tests/test_map_info_cpu.py, through GaussianMap.pose_information on the device: weak, three directions exactly open."""
import numpy as np
import pytest
import torch

from gsplatloc_amd.mapping import GaussianMap, MapConfig
from gsplatloc_amd.synthetic import write_replica_constant_twist
from tests.test_map_info_cpu import NEAR, PH, PK, PW, plane_case

pytestmark = pytest.mark.gpu
DEV = "cuda"
W, H, ITERS, N_B = 160, 120, 2000, 6


def _run(root, **cfg):
    from gsplatloc_amd.data import Parser
    from gsplatloc_amd.localizer import Localizer
    from gsplatloc_amd.my_gsplat import TrackerConfig

    parser = Parser("Replica", "room0", normalize=True, input_folder=str(root))
    depth, rgb, pose = parser.frame(0)
    loc = Localizer(parser.K, W, H, TrackerConfig(max_steps=ITERS), mode="map", map_config=MapConfig(**cfg))
    loc.reset(depth, rgb, pose)
    results = []
    for i in range(1, N_B):
        depth, rgb, pose = parser.frame(i)
        results.append(loc.track(depth, rgb, gt_c2w=pose))
    return loc, results


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    root = tmp_path_factory.mktemp("map_info_seq")
    write_replica_constant_twist(root, W, H, N_B, rot_deg=0.4, trans=0.01)
    return _run(root), _run(root, info=True)


def test_the_option_changes_nothing(runs):
    (plain, want), (loc, got) = runs
    assert torch.equal(loc.trajectory, plain.trajectory)
    assert [r.steps for r in got] == [r.steps for r in want] and [r.best_step for r in got] == [r.best_step for r in want]
    assert [r.added for r in got] == [r.added for r in want] and [r.map_size for r in got] == [r.map_size for r in want]
    assert [r.eT for r in got] == [r.eT for r in want] and not any(r.lost for r in got)
    assert loc.map.n_live == plain.map.n_live
    for a, b in ((loc.map.points, plain.map.points), (loc.map.point_colors, plain.map.point_colors)):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    assert all(r.weak is None and r.cov is None and r.info_used is None for r in want) and plain.map._info is None


def test_every_frame_reports_a_covariance(runs, capsys):
    _, (loc, results) = runs
    for i, r in enumerate(results, start=1):
        with capsys.disabled():
            print(f"[info] frame {i}: eT {r.eT:.3e} m eR {r.eR:.3e} deg, sigma_t {r.sigma_t} m sigma_r {r.sigma_r} deg, "
                  f"rows used {r.info_used}, min eig {r.info_min_eig:.3e}, weak {r.weak}")
    for i, r in enumerate(results, start=1):
        assert r.weak is False and r.info_used > 7 and r.info_min_eig >= 1e-3, (i, r.weak, r.info_used, r.info_min_eig)
        assert r.cov is not None and r.cov.shape == (6, 6) and r.cov.dtype == np.float64, i
        assert np.allclose(r.cov, r.cov.T, rtol=1e-9, atol=0.0), i
        assert np.all(np.linalg.eigvalsh(0.5 * (r.cov + r.cov.T)) > 0.0), (i, np.linalg.eigvalsh(r.cov))
        assert r.sigma_t > 0.0 and r.sigma_r > 0.0, i


def test_one_plane_is_weak_on_the_device():
    depth, means = plane_case()
    m = GaussianMap(PW, PH, MapConfig(info=True), DEV)
    assert m.insert_frame(torch.from_numpy(depth), torch.zeros(PH, PW, 3), PK, torch.eye(4)) == (PW * PH, PW * PH)
    assert np.array_equal(m.points.cpu().numpy(), means)
    info = m.pose_information(depth, PK, torch.eye(4), NEAR)
    assert info.used == info.tested == (PW - 2) * (PH - 2) and info.H[5, 5] == float(info.used)
    assert not info.H[2:5].any() and not info.g.any() and info.rss == 0.0  # omega_z, upsilon_x, upsilon_y: exactly open
    assert info.eigenvalues[0] == 0.0 and info.weak() and info.step() is None and info.covariance() is None
