"""GPU: Localizer(mode="map") with MapConfig.reloc -- every estimate is held against the map before it may touch it, and
a rejected one is tracked once more from the best-scoring pose of a grid around the start poses -- at 160x120, "ED", with
the settings and the yardstick of tests/test_gpu_map_localizer.py.

(a) The static room, the 6-frame constant twist of that file, reloc=True: no frame is relocalised or lost, and poses,
    step counts and added rows are bit for bit those of reloc=False run in the same process.  The map mode without the
    option is run twice first; if those two runs do not repeat bit for bit, the reloc run must lie within their
    difference (as tests/test_gpu_map_free_localizer.py does it).  Every frame's share agree / (agree + front) is
    printed.
(b) Real scoring, a stand-in tracker whose run() answers its start pose; everything else is real.  Frame 0 is taken 30
    degrees off the room's axis, frame 1 from that pose composed with one grid step, +1 x reloc_trans = 0.3 m along the
    camera's x (the pose is the grid's candidate 13 itself, so one candidate is exact).  The start is rejected; the
    winner is the candidate the mirror names on host copies of the map; the frame is accepted with relocalised=True
    and its rows are inserted at that pose.  The mirror's margin over the runner-up is printed.
(c) The real tracker, with a jump.  A constant-twist sequence of 3 + m + 2 frames (0.4 degrees and 1 cm per frame), of
    which frames 0, 1, 2, 2 + m and 3 + m are fed: the camera jumps by m steps.  The jump was meant to break the run
    without the option -- the smallest m of 4, 8, 16, 32 whose final absolute error exceeds 10 times the bound of the map
    test, twice the running sum of the yardstick's pair errors -- and no m does: the tracker's basin is wider than this
    scene can leave (at m = 32 the camera turns 12.8 degrees and moves 32 cm between two frames, and two thirds of the
    map are still in the image).  So, with m = 32 and a grid whose second level reaches half the jump, the test asserts
    only that nothing is relocalised or lost and that poses, step counts and added rows equal the run without the option
    bit for bit.  The errors are printed.
(d) evaluate_room(..., map_reloc=True) on the static sequence: relocalised_frames == 0, one agree share per frame, and
    a plain report has neither key.

Measured on the MI355X.  (a) the two runs without the option repeat bit for bit -- steps 349, 648, 321, 572, 356, added
rows 120, 120, 145, 135, 130 -- and the reloc run gives the same bits; (tested, agree, front) per frame (18991, 18991, 0),
(18798, 18798, 0), (18675, 18675, 0), (18593, 18593, 0), (18488, 18488, 0): every share is 1.  (b) the start scores (19200, 2044, 6940), share 0.2275; the winner is candidate 13
with (17760, 17760, 0), the runner-up's agree - front is 8160, 9600 rows less; 1320 rows added.  (c) without the option,
final absolute error and bound 2 sum eT_i at m = 4: 7.8e-4 / 9.8e-3 m; m = 8: 9.9e-4 / 1.3e-2; m = 16: 1.8e-3 / 2.1e-2;
m = 32: 4.1e-3 / 4.4e-2 -- under a tenth of the bound every time, no frame lost; with the option the same bits, the jump
frame's verdict (tested, agree, front) 17983 / 17138 / 15577 / 12986 rows tested, all of them agreeing, none in front.
NOTES.md, "Relocalisation", has these, the shares of the free-space panel sequence and the launch cost."""
import numpy as np
import pytest
import torch

from gsplatloc_amd.localizer import Localizer, reloc_candidates
from gsplatloc_amd.mapping import MapConfig
from gsplatloc_amd.my_gsplat import TrackerConfig
from gsplatloc_amd.my_gsplat.trainer import TrackResult
from gsplatloc_amd.synthetic import replica_intrinsics, room_depth, write_replica_constant_twist
from tests import map_score_ref as ref
from tests.pose_ref import axis_angle
from tests.test_gpu_map_localizer import ITERS, N_B, H, W, _yardstick
from tests.test_gpu_map_view_localizer import _bits, _run

pytestmark = pytest.mark.gpu
F32 = np.float32
STEP_B, YAW_B = 0.3, -30.0
M_JUMP = 32  # the largest jump tried; none of 4, 8, 16, 32 breaks the run without the option (the docstring, (c))


def _share(r):
    return r.agree / (r.agree + r.front) if r.agree + r.front > 0 else None


@pytest.fixture(scope="module")
def seq_b(tmp_path_factory):
    root = tmp_path_factory.mktemp("reloc_seq_b")
    write_replica_constant_twist(root, W, H, N_B, rot_deg=0.4, trans=0.01)
    return root


def test_reloc_changes_nothing_on_the_static_room(seq_b, capsys):
    first, second = _run(seq_b, N_B, MapConfig()), _run(seq_b, N_B, MapConfig())
    reloc = _run(seq_b, N_B, MapConfig(reloc=True))
    (p1, s1, a1), (p2, s2, a2), (pr, sr, ar) = _bits(first), _bits(second), _bits(reloc)
    repeats = np.array_equal(p1, p2) and s1 == s2 and a1 == a2
    d_pose = float((first["traj"] - second["traj"]).abs().max())
    d_steps, d_added = max(abs(a - b) for a, b in zip(s1, s2)), max(abs(a - b) for a, b in zip(a1, a2))
    r_pose = float((first["traj"] - reloc["traj"]).abs().max())
    r_steps, r_added = max(abs(a - b) for a, b in zip(s1, sr)), max(abs(a - b) for a, b in zip(a1, ar))
    res = reloc["results"]
    with capsys.disabled():
        print(f"[reloc] (a) without the option twice: repeats bit for bit {repeats}; largest difference pose {d_pose:.3e}, "
              f"steps {d_steps}, added {d_added}; reloc against the first: pose {r_pose:.3e}, steps {r_steps}, added "
              f"{r_added}; steps {s1} / {sr}, added {a1} / {ar}")
        print(f"[reloc] (a) agree share per frame {['%.4f' % _share(r) for r in res]}, (tested, agree, front) "
              f"{[(r.tested, r.agree, r.front) for r in res]}")
    assert all(r.relocalised is None and r.tested is None and r.agree is None and r.front is None
               for r in first["results"])
    assert [r.relocalised for r in res] == [False] * (N_B - 1) and not any(r.lost for r in res)
    assert all(r.tested >= (W * H) // 16 and r.agree >= MapConfig().reloc_min_agree * (r.agree + r.front) for r in res)
    if repeats:
        assert np.array_equal(pr, p1) and sr == s1 and ar == a1
    else:
        assert r_pose <= d_pose and r_steps <= d_steps and r_added <= d_added


class _StartTracker:
    """Stands in for GraphTracker: run() answers the pose it was started from."""
    made = []

    def __init__(self, N, W_, H_, config, device, render_mode):
        self.N, self.starts = N, []
        _StartTracker.made.append(self)

    def load_frame(self, tar_points, colors, scales, src_depth, tar_c2w, src_c2w, K, pixels=None):
        assert tar_points.shape == (self.N, 3)
        self.starts.append(tar_c2w.clone())

    def run(self):
        start = self.starts[-1]
        return TrackResult(best_loss=0.25, steps=12, final_c2w=start.clone(), best_c2w=start.clone(), best_step=7)


def test_real_scoring_names_the_candidate_that_is_the_frames_pose(capsys):
    K = replica_intrinsics(W, H)
    intr = tuple(float(F32(a)) for a in (K[0, 0], K[1, 1], K[0, 2], K[1, 2]))
    pose0 = torch.eye(4)
    pose0[:3, :3] = axis_angle((0.0, 1.0, 0.0), YAW_B).float()
    cfg = MapConfig(reloc=True, reloc_trans=STEP_B)
    cands = reloc_candidates([pose0], cfg.reloc_rot_deg, cfg.reloc_trans, cfg.reloc_levels)
    exact = 1 + 6 * cfg.reloc_levels  # the first shift: +1 x reloc_trans along x
    pose1 = cands[exact]
    assert abs(float((torch.linalg.inv(pose0) @ pose1)[0, 3]) - STEP_B) < 1e-6
    gen = torch.Generator().manual_seed(5)
    frames = [(room_depth(W, H, K, p), torch.randint(0, 255, (H, W, 3), generator=gen).float()) for p in (pose0, pose1)]
    _StartTracker.made = []
    tcfg = TrackerConfig(max_steps=ITERS)
    loc = Localizer(K, W, H, tcfg, normalize=False, motion="hold", tracker_factory=_StartTracker, mode="map",
                    map_config=cfg)
    loc.reset(*frames[0], pose0)
    n0 = loc.map.n_live
    rows = loc.map.points.cpu().numpy().copy()
    r = loc.track(*frames[1], gt_c2w=pose1)
    # the mirror on host copies of the map as it was when the frame came
    w2cs = np.stack([ref.w2c_of(c.numpy()) for c in cands])
    want = ref.score(rows, w2cs, intr, frames[1][0].numpy(), F32(loc.map.keep), F32(loc.map.beyond), tcfg.gs.near_plane)
    margins = (want[:, 1] - want[:, 2]).tolist()
    winner = margins.index(max(margins))
    runner_up = sorted(margins)[-2]
    start_share = want[0, 1] / (want[0, 1] + want[0, 2])
    with capsys.disabled():
        print(f"[reloc] (b) start (tested, agree, front) {want[0].tolist()}, share {start_share:.4f}; winner {winner} "
              f"{want[winner].tolist()}, margin {margins[winner]} against the runner-up's {runner_up}: "
              f"{margins[winner] - runner_up} rows; added {r.added}")
    assert n0 == W * H and start_share < cfg.reloc_min_agree  # the start is rejected
    assert winner == exact and margins[winner] > runner_up
    starts = [s for t in _StartTracker.made for s in t.starts]
    assert len(starts) == 2 and torch.equal(starts[0].cpu(), pose0) and torch.equal(starts[1].cpu(), cands[winner])
    assert (r.lost, r.relocalised, r.steps) == (False, True, 24) and torch.equal(r.c2w.cpu(), pose1) and r.eT == 0.0
    assert (r.tested, r.agree, r.front) == tuple(want[winner].tolist()) and r.front == 0 and r.agree == r.tested
    # its rows went in at that pose: from there every one of them sits on the surface its own pixel observes
    assert r.added > 0 and r.map_size == n0 + r.added == loc.map.n_live
    new = loc.map.points[n0:].cpu().numpy()
    at = ref.score(new, w2cs[winner][None], intr, frames[1][0].numpy(), F32(loc.map.keep), F32(loc.map.beyond),
                   tcfg.gs.near_plane)[0]
    assert at.tolist() == [r.added, r.added, 0]
    assert np.array_equal(loc.map.points[:n0].cpu().numpy().view(np.uint32), rows.view(np.uint32))


def _run_fed(root, indices, map_config):
    """Localizer(mode="map") over the frames ``indices`` of the sequence, the first with its pose."""
    from gsplatloc_amd.data import Parser

    parser = Parser("Replica", "room0", normalize=True, input_folder=str(root))
    depth, rgb, pose = parser.frame(indices[0])
    loc = Localizer(parser.K, W, H, TrackerConfig(max_steps=ITERS), mode="map", map_config=map_config)
    loc.reset(depth, rgb, pose)
    gts, results = [pose], []
    for i in indices[1:]:
        depth, rgb, pose = parser.frame(i)
        results.append(loc.track(depth, rgb, gt_c2w=pose))
        gts.append(pose)
    return dict(traj=loc.trajectory, gts=torch.stack(gts), results=results)


def test_a_jump_the_tracker_absorbs_is_not_relocalised(tmp_path, capsys):
    m = M_JUMP
    write_replica_constant_twist(tmp_path, W, H, 3 + m + 2, rot_deg=0.4, trans=0.01)
    fed = [0, 1, 2, 2 + m, 3 + m]
    plain = _run_fed(tmp_path, fed, MapConfig())
    reloc = _run_fed(tmp_path, fed, MapConfig(reloc=True, reloc_rot_deg=0.4 * m / 4.0, reloc_trans=0.01 * m / 4.0))
    err = (reloc["traj"][:, :3, 3] - reloc["gts"][:, :3, 3]).norm(dim=1).tolist()
    res = reloc["results"]
    bound = 2.0 * sum(_yardstick(tmp_path, 3 + m + 2))
    with capsys.disabled():
        print(f"[reloc] (c) m {m}: bound 2 sum eT_i over the whole sequence {bound:.3e} m (printed, not asserted)")
        print(f"[reloc] (c) m {m}: abs error per fed frame {['%.3e' % e for e in err]}, steps {[r.steps for r in res]}, "
              f"(tested, agree, front) {[(r.tested, r.agree, r.front) for r in res]}, agree share "
              f"{['%.4f' % _share(r) for r in res]}")
    assert [r.relocalised for r in res] == [False] * 4 and not any(r.lost for r in res)
    assert not any(r.lost for r in plain["results"]) and all(r.relocalised is None for r in plain["results"])
    (pp, sp, ap), (pr, sr, ar) = _bits(plain), _bits(reloc)
    assert np.array_equal(pr, pp) and sr == sp and ar == ap


def test_the_evaluation_driver_reports_relocalisation(seq_b):
    from gsplatloc_amd.data import Parser
    from gsplatloc_amd.eval import evaluate_room

    parser = Parser("Replica", "room0", normalize=True, input_folder=str(seq_b))
    r = evaluate_room(parser, ITERS, None, sequential=True, map_mode=True, map_reloc=True)
    assert r["reloc"] is True and r["relocalised_frames"] == 0 and r["lost_frames"] == 0 and r["frames"] == N_B - 1
    assert len(r["agree_share_per_frame"]) == N_B - 1 and all(0.0 < s <= 1.0 for s in r["agree_share_per_frame"])
    plain = evaluate_room(parser, ITERS, None, sequential=True, map_mode=True)
    assert "relocalised_frames" not in plain and "agree_share_per_frame" not in plain and "reloc" not in plain
